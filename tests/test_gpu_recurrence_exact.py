"""Every recurrent kernel against the exact integer-grid reference (tests/exact_net.py).

On these cases every product and partial sum of every hidden layer is a small integer, so fp32 accumulation is exact
in any order, for any K split, on any MFMA shape, with fp32, three-term bfloat16 or float16 operands: the rows of
W h + b, hActsFor and hActsBack of every frame of every utterance must be BIT-equal to the float64 oracle -- no
tolerance, no retry, no second kernel to compare with.  Every (0, maxAct) mask is then the same on both sides, the
backward pass is a fixed linear map of the CTC delta, and it is checked per frame: a row of delta_1 whose reference row
is exactly zero must be exactly zero; for the others rho_dev = max over frames of ||got - ref|| / ||ref|| must stay
within 16 x rho_32 (the same statistic of a float32 NumPy restatement of the backward pass against the float64 one,
computed at run time) and within 1e-4 (TOL_MASKED of tests/test_gpu_fullsize.py); the same rule per gradient tensor
with the relative Frobenius norm.

fp16=True (the f16 rows).  Forward: as above, and every 16-bit shadow the GEMMs read -- the float16 and bfloat16 copies of
hActs[0..NL], the bfloat16 copies of hActsFor / hActsBack -- is the rounding of the exact reference bit for bit, padding
columns zero; the hidden ReLU layers have no fp32 copy in this configuration, so this is their only check.  Backward: the
masks being the reference's, the pass is a fixed linear map of the CTC delta with roundings at fixed points, which
exact_net.Rounding names and exact_net.reference(mixed=) restates.  M64 is that restatement accumulating in float64, M32
the same in float32.  Against M64:
  * zeros: an element of deltasFor / deltasBack behind a closed mask is exactly zero; a frame of delta_1 that is zero in
    M64 is zero;
  * per gradient tensor, rel_fro(device, M64) <= 16 x e_ref, e_ref = the largest rel_fro(M32, M64) over seeds 0..7 of the
    row's shape (computed here, on the host; several seeds because one rounding flip moves it and the device's flips need
    not be NumPy's), floored at 2^-24 (the results are stored in fp32); and <= 5e-2 against the unrounded oracle, the
    configuration's own bar;
  * per frame, the same rule for deltasFor, deltasBack (fp32) and delta_1 (its bfloat16 shadow against M64's);
  * per element: at most 1e-3 of the elements of a bfloat16 delta shadow (deltasFor, deltasBack, delta_1, delta_2) differ
    from M64's, every frame of every utterance counted (M32 alone stays within 2e-4: tests/test_exact_net_cpu.py, which
    also shows that every misplaced rounding is reported by these rules at these bounds).
On these networks the B operands (weights, features, hF, hB, their sum; a ReLU layer's output unless it has an odd value
above 256) are bfloat16 values already: it is the roundings of the DELTAS, the bias gradients among them, that the
backward rules pin.

The matrix (exact_net.GPU_CASES) follows launch_recurrent_one / launch_recurrent of csrc/recurrent.hip: the sentinel /
VALU kernel (4- and 8-utterance instantiations), the flag kernel as one and as two chains, the 16-bit exchange kernel,
the tiled kernel in its three forms (units x both tiles per CU; one / two tiles per sub-chain) at the large and, on
request, the small layers, the one-slab-per-CU kernel with 1 / 2 / 4 tiles per wave, its generic instantiation at
layer sizes without a specialised kernel, the per-step fallback, and the cuts of launch_recurrent (32 + 8, 64 + 16,
never, 128 + 22).  recurrentPath() only tells persistent (1) from per-step (3): which kernel a persistent launch
runs follows from (H, B, operand type, SCTC_REC_VARIANT) by rec_plan / rec_cut (csrc/recurrent_plan.h), not from an
observable of the engine; tests/test_recurrence_plan_cpu.py asserts for every row of the matrix that the plan's first
candidate is the family the row's id names, and for the cut rows the launch sizes.  SCTC_REC_TCFG is read once per
process and is left out.

What this file does not cover: the arithmetic error of the forward recurrence on non-integer data (the oracle tests of
test_gpu_brnn / test_gpu_fullsize / gpu_fuzz keep that; for the fp16-operand configuration tests/test_gpu_fp16.py, at
that configuration's tolerances), a rounding of a B operand of a backward GEMM that changes its value (see above), and
utterances longer than 16 frames: these +-1 networks amplify a delta by about 2.3 per BPTT step, and beyond that the
float32 restatement itself leaves the float64 one (6.6e-3 on dW1 at 40 frames).

OBSERVED (MI355X)
-----------------
Per case: frames; per direction the shares of (unit, frame) pairs open / at 0 / at maxAct and the numbers of
pre-activations (steps with a recurrent term) exactly 0 and exactly maxAct; rho_dev, rho_32 and their ratio for delta_1;
the largest ratio over delta_1 and all gradient tensors, and where.  Every forward buffer was bit-equal in every case;
the largest ratio seen is 7.0 (dW3, the 9 x 64 output layer over 1018 frames: BLAS's float32 sum is unusually good there,
4.8e-8, the device's 3.4e-7), against the margin of 16 (rho_32 is the host BLAS's error, so the ratios move a little with
the host's sgemm kernels; the device's side is deterministic);the largest rho_dev 3.7e-6, the largest tensor error 3.9e-7.

case                          frm  F o/z/c      F==0 F==mx  B o/z/c      B==0 B==mx  rho_dev   rho_32    ratio  worst
s4-H512-B1-v0-f32              16  .162/.532/.307    67    60  .166/.528/.306    88    52  2.25e-07  2.41e-07   0.93   2.88 db3
s4-H512-B3-v0-f32              33  .168/.532/.300   132   119  .173/.536/.291   138   100  3.67e-07  3.01e-07   1.22   1.44 dWb
s4-H1824-B1-v0-f32             16  .165/.528/.307   199   189  .163/.526/.311   221   215  2.05e-07  2.49e-07   0.83   1.46 db2
s4-H1824-B3-v0-f32             33  .169/.536/.295   445   406  .172/.532/.297   466   392  2.90e-07  2.51e-07   1.16   1.46 db3
s8-H1024-B7-v43-f32            74  .175/.533/.292   641   483  .173/.537/.290   606   482  2.56e-07  2.71e-07   0.95   2.01 db3
q1-H512-B4-v0-f32              49  .165/.533/.302   186   164  .169/.531/.300   185   161  3.08e-07  4.22e-07   0.73   1.51 db2
q1-H1024-B11-v0-f32            79  .189/.541/.270   600   468  .190/.539/.272   676   527  2.43e-07  2.43e-07   1.00   1.23 dWb
q1-H1824-B4-v0-f32             43  .171/.533/.296   649   481  .174/.536/.290   590   523  2.31e-07  2.07e-07   1.12   1.19 db2
q1-H1824-B11-v0-f32            90  .183/.541/.276  1285  1075  .185/.537/.278  1373  1070  2.41e-07  2.26e-07   1.07   1.44 db2
q1-H1824-B16-v0-f32           146  .181/.539/.281  2205  1701  .183/.537/.280  2138  1773  2.81e-07  3.23e-07   0.87   1.49 db2
q1-H2048-B16-v0-f32           104  .199/.543/.258  1865  1336  .199/.544/.256  1866  1393  2.19e-07  2.12e-07   1.04   1.43 db2
mh-H512-B6-v0-f16              72  .170/.535/.295   290   223  .170/.533/.297   316   252  fp16 operands: below
mh-H512-B16-v0-f16            112  .191/.536/.273   458   397  .190/.540/.270   438   392  fp16 operands: below
mh-H1824-B6-v0-f16             68  .174/.534/.292   954   778  .171/.538/.290   996   813  fp16 operands: below
mh-H1824-B16-v0-f16           146  .181/.539/.281  2205  1701  .183/.537/.280  2138  1773  fp16 operands: below
s4-H512-B2-v0-f16              17  .174/.526/.300    62    60  .173/.524/.303    53    78  fp16 operands: below
q2-H512-B24-v0-f16            190  .189/.543/.268   838   651  .190/.539/.271   800   643  fp16 operands: below
mh-H1024-B12-v0-f16           108  .183/.538/.279   906   746  .182/.539/.279   929   760  fp16 operands: below
mh-H2048-B9-v0-f16             78  .181/.537/.282  1321   964  .181/.538/.281  1262  1103  fp16 operands: below
q1-H512-B5-v0-f16              55  .173/.538/.289   241   194  .175/.534/.291   216   177  fp16 operands: below
slab-H512-B40-v0-f16          290  .194/.541/.265  1217   878  .194/.541/.265  1201  1020  fp16 operands: below
fallback-H512-B7-v3-f16        89  .167/.535/.298   377   301  .172/.531/.297   387   304  fp16 operands: below
below-tl-H200-B12-v0-f16       86  .187/.505/.308   127    71  .191/.500/.309   119   115  fp16 operands: below
t-ug1-H1824-B17-v0-f32        116  .196/.542/.263  1786  1367  .193/.544/.262  1716  1359  2.23e-07  2.61e-07   0.86   1.17 db3
t-ug1-H1824-B24-v0-f32        240  .179/.534/.286  3544  2948  .181/.535/.284  3599  2838  2.64e-07  2.35e-07   1.13   1.44 db2
t-ug1-H1824-B32-v0-f32        232  .192/.543/.265  3531  2765  .192/.541/.267  3351  2693  3.07e-07  2.50e-07   1.23   1.54 db2
t-ug1-H2048-B17-v0-f32        144  .185/.541/.275  2424  2019  .185/.537/.278  2468  1936  2.50e-07  2.26e-07   1.11   4.00 db3
t-ug1-H2048-B24-v0-f32        196  .187/.539/.274  3368  2554  .186/.541/.273  3401  2610  2.50e-07  2.41e-07   1.04   2.44 db3
t-ug1-H2048-B32-v0-f32        265  .187/.537/.276  4566  3602  .187/.538/.275  4383  3615  2.58e-07  2.76e-07   0.94   4.71 db3
q2-H512-B17-v0-f32            130  .195/.539/.266   618   429  .193/.540/.267   564   454  3.62e-07  4.25e-07   0.85   1.54 db2
q2-H512-B32-v0-f32            250  .191/.540/.269  1139   822  .190/.541/.269  1149   826  2.94e-07  7.12e-07   0.41   1.39 db2
q2-H1024-B17-v0-f32           150  .185/.540/.275  1221  1014  .187/.539/.274  1278  1041  2.56e-07  2.59e-07   0.99   1.52 db2
q2-H1024-B32-v0-f32           227  .197/.541/.262  2026  1525  .196/.543/.261  1973  1566  2.67e-07  2.50e-07   1.07   1.55 db3
q2-H1824-B24-v51-f32          240  .179/.534/.286  3544  2948  .181/.535/.284  3599  2838  2.64e-07  2.35e-07   1.13   1.44 db2
t-1tile-H1824-B33-v0-f32      224  .196/.544/.260  3489  2646  .196/.543/.262  3449  2648  2.32e-07  2.30e-07   1.01   1.68 db3
t-1tile-H1824-B64-v0-f32      405  .201/.546/.254  6151  4796  .201/.545/.254  6292  4812  2.28e-07  2.52e-07   0.90   1.39 db3
t-1tile-H2048-B33-v0-f32      214  .201/.544/.255  3725  2754  .201/.544/.256  3757  2790  2.28e-07  3.05e-07   0.75   1.33 db2
t-1tile-H2048-B64-v0-f32      447  .196/.542/.261  7877  6018  .197/.542/.261  7798  6009  2.24e-07  2.79e-07   0.80   1.52 db3
t-2tile-H1824-B100-v0-f32     654  .200/.545/.255 10345  7653  .201/.544/.255 10185  7774  2.52e-07  3.18e-07   0.79   1.34 db3
t-2tile-H1824-B128-v0-f32     823  .200/.545/.255 12822  9707  .199/.545/.256 12679  9578  2.49e-07  2.43e-07   1.03   4.69 db3
t-2tile-H2048-B100-v0-f32     682  .199/.543/.258 11963  9065  .199/.544/.257 12206  8913  2.57e-07  2.57e-07   1.00   1.27 db2
t-2tile-H2048-B128-v0-f32     856  .199/.543/.257 14894 11444  .200/.544/.257 15211 11326  2.97e-07  2.43e-07   1.22   1.26 db2
t-cut64-H1824-B80-v0-f32      549  .198/.543/.259  8503  6382  .197/.542/.261  8383  6389  2.75e-07  2.61e-07   1.05   1.25 db2
t-nocut-H1824-B80-v45-f32     549  .198/.543/.259  8503  6382  .197/.542/.261  8383  6389  2.75e-07  2.61e-07   1.05   1.25 db2
t-small-H512-B40-v50-f32      290  .194/.541/.265  1217   878  .194/.541/.265  1201  1020  3.42e-07  3.33e-07   1.03   1.40 db2
t-small-H512-B100-v50-f32     677  .197/.545/.258  2950  2269  .199/.543/.258  2990  2270  3.65e-07  2.92e-07   1.25   1.25 d1
t-small-H1024-B40-v50-f32     239  .207/.546/.248  2107  1573  .205/.547/.248  2131  1586  2.93e-07  2.54e-07   1.15   1.27 db2
t-small-H1024-B100-v50-f32    662  .201/.544/.255  5946  4397  .201/.545/.254  5871  4405  2.72e-07  4.13e-07   0.66   1.29 db2
slab-H512-B9-v1-f32            86  .181/.541/.279   378   297  .184/.538/.279   374   288  4.08e-07  2.66e-07   1.53   2.01 db3
slab-H512-B40-v1-f32          290  .194/.541/.265  1217   878  .194/.541/.265  1201  1020  3.07e-07  3.33e-07   0.92   1.40 db2
slab-H512-B100-v1-f32         677  .197/.545/.258  2950  2269  .199/.543/.258  2990  2270  3.63e-07  2.92e-07   1.24   1.24 d1
cut32-H512-B40-v0-f32         290  .194/.541/.265  1217   878  .194/.541/.265  1201  1020  3.42e-07  3.33e-07   1.03   1.40 db2
generic-H96-B5-v0-f32          55  .175/.530/.295    37    35  .166/.537/.298    46    33  8.06e-07  5.18e-07   1.56   1.75 dW3
generic-H96-B40-v0-f32        270  .203/.540/.256   214   158  .202/.545/.253   226   167  4.42e-07  4.75e-07   0.93   3.50 dW3
generic-H96-B128-v0-f32       851  .199/.546/.255   680   524  .200/.542/.257   661   506  7.41e-07  6.40e-07   1.16   6.30 dW3
generic-H132-B5-v0-f32         57  .170/.532/.298    63    53  .173/.539/.288    47    41  3.19e-07  5.89e-07   0.54   2.50 db3
generic-H132-B40-v0-f32       270  .196/.543/.261   314   224  .197/.539/.263   328   269  5.61e-07  5.19e-07   1.08   3.94 dW3
generic-H132-B128-v0-f32      845  .201/.546/.253   941   745  .201/.544/.255   973   710  5.76e-07  5.13e-07   1.12   4.78 db3
fallback-H512-B7-v3-f32        89  .167/.535/.298   377   301  .172/.531/.297   387   304  4.21e-07  3.62e-07   1.16   1.33 db2
fallback-H96-B20-v3-f32       146  .196/.543/.261   117   105  .201/.537/.262   136   107  4.60e-07  3.98e-07   1.16   3.29 dW3
two-launches-H64-B150-v0-f32 1018  .198/.537/.265   550   407  .199/.546/.256   575   433  3.66e-06  2.67e-06   1.37   7.01 dW3
below-tl-H200-B5-v0-f32        55  .160/.508/.332    89    67  .160/.500/.341    73    81  5.42e-07  3.95e-07   1.37   1.49 db4
bf16x3-H512-B8-v0-bf16x3       94  .172/.536/.292   398   298  .170/.535/.294   360   315  4.25e-07  3.20e-07   1.33   2.05 dWf

The fp16-operand rows' backward pass (same run).  worst: the statistic with the largest e_dev / max(e_ref, 2^-24) over the
gradient tensors and the per-frame errors of deltasFor (dF), deltasBack (dB) and delta_1's shadow; largest tensor error;
d1: per-frame error of delta_1's shadow, device / e_ref; the shares of the four bfloat16 delta shadows' elements that differ
from M64's; the largest tensor error against the unrounded oracle (bar 5e-2).  No element behind a closed mask and no zero
frame of delta_1 was non-zero in any row.  The device agrees with the model to fp32 accumulation accuracy (bias gradients
included: they are sums of the bfloat16 deltas), the 16-bit exchange rows without a single differing shadow element; on the
fp32-recurrence rows it makes a few rounding flips of its own (one or two elements of a shadow; the fallback row's flip is
its 3.75), as M32 does on other seeds -- which is what e_ref's eight seeds are for (e.g. 8.0e-04 for d1 at mh-H1024-B12).

case                         worst e_dev     e_ref     ratio  largest tensor  d1 dev/e_ref      share dF      dB      d1      d2   vs exact
mh-H512-B6-v0-f16            db1  4.36e-08  4.23e-08  0.73   db1  4.4e-08   0.0e+00/0.0e+00         0       0       0       0   7.0e-03
mh-H512-B16-v0-f16           dW1  4.55e-08  6.53e-08  0.70   dW1  4.6e-08   0.0e+00/0.0e+00         0       0       0       0   7.6e-03
mh-H1824-B6-v0-f16           db1  4.13e-08  3.94e-08  0.69   dW1  4.1e-08   0.0e+00/0.0e+00         0       0       0       0   7.3e-03
mh-H1824-B16-v0-f16          dW1  4.59e-08  5.33e-08  0.77   dW1  4.6e-08   0.0e+00/0.0e+00         0       0       0       0   6.7e-03
s4-H512-B2-v0-f16            dB   1.15e-07  1.59e-07  0.72   dW1  2.7e-08   0.0e+00/1.3e-05         0       0       0       0   3.1e-03
q2-H512-B24-v0-f16           dF   1.86e-07  1.67e-07  1.11   dW1  4.9e-08   0.0e+00/1.2e-04         0       0       0       0   3.7e-03
mh-H1024-B12-v0-f16          dB   2.93e-08  3.11e-08  0.49   dW1  3.7e-08   0.0e+00/8.0e-04         0       0       0       0   8.1e-03
mh-H2048-B9-v0-f16           dW1  4.33e-08  5.10e-08  0.73   dW1  4.3e-08   0.0e+00/0.0e+00         0       0       0       0   7.1e-03
q1-H512-B5-v0-f16            dF   1.73e-07  1.87e-07  0.92   dWb  5.7e-06   7.8e-05/8.0e-04         0  3.6e-5  7.1e-5       0   3.7e-03
slab-H512-B40-v0-f16         dF   1.45e-07  1.36e-07  1.07   dWb  2.4e-06   1.6e-05/5.0e-04         0  6.7e-6  6.7e-6       0   3.0e-03
fallback-H512-B7-v3-f16      dWf  5.36e-05  1.43e-05  3.75   dWf  5.4e-05   3.7e-04/6.7e-04    2.2e-5  2.2e-5  4.4e-5       0   2.8e-03
below-tl-H200-B12-v0-f16     dF   1.55e-07  1.58e-07  0.98   dW2  3.1e-08   0.0e+00/0.0e+00         0       0       0       0   3.6e-03
"""
import numpy as np
import pytest

from oracle import brnn as obrnn
from tests import exact_net as en
from tests.test_gpu_brnn import _note, _packed_rowbase, make_net
from tests.test_gpu_fp16 import make_net16

pytestmark = pytest.mark.gpu

TOL_MASKED = 1e-4        # the project's masked-oracle bar (tests/test_gpu_fullsize.py)
MARGIN = 16.0            # rho_dev <= MARGIN * rho_32: room for a summation order and blocking other than BLAS's, and
#                          for the device's fp32 softmax under the CTC delta
TOL_FP16_EXACT = 5e-2    # the fp16-operand configuration's stated bar against the unrounded oracle (tests/test_gpu_fp16.py)
TWICE = "t-cut64-H1824-B80-v0-f32"      # this case runs the same step twice: bit-identical gradients


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nnets import brnnet
    return brnnet


def _build(brnnet, c, case):
    if c.mode == "f16":
        net = make_net16(brnnet, case.dims, case.params, maxUtts=c.B)
        assert net.maxAct == case.max_act
        return net
    return make_net(brnnet, case.dims, case.params, maxUtts=c.B, max_act=case.max_act, gemm=c.mode)


def _per_utt(X, rows, H):
    """packed device matrix [N][Hp] -> per utterance (H, T_b), caller's order"""
    return [X[r, :H].T for r in rows]


def _values16(net, which, kind):
    """a 16-bit shadow of the engine as float64 values [N][Hp]; the engine must call it the type `kind`"""
    bits, said = net.debugBuffer16(which)
    assert said == kind and bits.dtype == np.uint16, (which, said, bits.dtype)
    if kind == "float16":
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _describe(got, ref, names, Ts, rank):
    """where a forward mismatch sits: buffer, utterance (caller index / length rank / length), frames, units"""
    out = []
    for n in names:
        for b, (g, r) in enumerate(zip(got[n], ref[n])):
            bad = np.float32(g) != np.float32(r)
            if bad.any():
                u, t = np.nonzero(bad)
                out.append("%s utt %d (rank %d, T=%d): %d values, frames %s, units %d..%d (%d distinct; 16-blocks %s), first got %r want %r"
                           % (n, b, rank[b], Ts[b], bad.sum(), sorted(set(t.tolist()))[:16], u.min(), u.max(), len(set(u.tolist())),
                              sorted(set((u // 16).tolist()))[:12], float(g[u[0], t[0]]), float(r[u[0], t[0]])))
    return "\n".join(out[:24])


def _device_grads(net, NL):
    g = {"W": [net.grad[i][0].copy_to_host().astype(np.float64) for i in range(NL + 1)],
         "b": [net.grad[i][1].copy_to_host().astype(np.float64).reshape(-1, 1) for i in range(NL + 1)],
         "Wf": net.grad[NL + 1][0].copy_to_host().astype(np.float64),
         "Wb": net.grad[NL + 2][0].copy_to_host().astype(np.float64)}
    return g


@pytest.mark.parametrize("c", en.GPU_CASES, ids=lambda c: c.id)
def test_recurrence_exact(mods, monkeypatch, c):
    brnnet = mods
    case = en.gpu_case(c)
    D, A, H, NL, TL, Tmax = case.dims
    Ts, B = case.Ts, c.B
    monkeypatch.delenv("SCTC_GEMM", raising=False)
    monkeypatch.setenv("SCTC_REC_VARIANT", c.variant)
    net = _build(brnnet, c, case)
    costs, _, skips = net.costAndGradBatch(case.datas, case.labs)
    costs, skips = costs.copy(), skips.copy()
    assert net.recurrentPath() == c.rec_path
    hF, hB, Z = net.debugBuffer(100), net.debugBuffer(101), net.debugBuffer(102)
    fp32 = c.mode != "f16"
    grads = _device_grads(net, NL)
    if fp32:
        acts = [net.debugBuffer(i) for i in range(1, NL + 1)]
        d1 = net.debugBuffer(200)
    else:
        dF, dBk = net.debugBuffer(201), net.debugBuffer(202)
        # the 16-bit shadows, as values: the forward operands (float16 and bfloat16 copies of hActs[i], bfloat16 of hF / hB)
        # and the backward pass's bfloat16 deltas
        fwd16 = [("act%d.f16" % i, i, "float16", i) for i in range(NL + 1)]
        fwd16 += [("act%d.bf16" % i, 50 + i, "bfloat16", i) for i in range(NL + 1)] + [("hF.bf16", 100, "bfloat16", "hF"), ("hB.bf16", 101, "bfloat16", "hB")]
        sh16 = {name: _values16(net, which, kind) for name, which, kind, _ in fwd16}
        sh16.update({k: _values16(net, which, "bfloat16") for k, which in (("d1", 200), ("dF", 201), ("dB", 202), ("d2", 203))})
    # packed rows -> utterances: the engine orders by length (stable, longest first); frame t of rank r is row rowbase[t] + r
    order = sorted(range(B), key=lambda b: -Ts[b])
    rank = np.empty(B, dtype=np.int64)
    rank[order] = np.arange(B)
    rb = _packed_rowbase(Ts)
    rows = [rb[:Ts[b]] + rank[b] for b in range(B)]
    assert Z.shape[0] == sum(Ts) and sorted(np.concatenate(rows).tolist()) == list(range(sum(Ts)))
    ref = en.reference(case)

    # ---- forward: bit equality
    got = {"z": _per_utt(Z, rows, H), "hF": _per_utt(hF, rows, H), "hB": _per_utt(hB, rows, H)}
    names = ("z", "hF", "hB")
    if fp32:
        for i in range(1, NL + 1):
            got["act%d" % i] = _per_utt(acts[i - 1], rows, H)
            ref["act%d" % i] = ref["acts"][i]
            names += ("act%d" % i,)
    n_bad = en.forward_rows_differing(got, ref, names=names)
    if n_bad:
        pytest.fail("%s: %d of %d (utterance, frame) rows differ from the exact reference\n%s"
                    % (c.id, n_bad, sum(Ts), _describe(got, ref, names, Ts, rank)))
    for n in names:
        for g, r in zip(got[n], ref[n]):
            np.testing.assert_array_equal(np.float32(g), np.float32(r))
    for name, X in (("z", Z), ("hF", hF), ("hB", hB)):
        assert X.shape[1] % 32 == 0 and X.shape[1] >= H
        assert not X[:, H:].any(), "%s: padding columns of %s are not zero" % (c.id, name)
    if not fp32:
        # the hidden ReLU layers exist as shadows only: every shadow is the rounding of the exact reference, bit for bit
        # (the values are integers <= 2048 -- float16 holds them all, bfloat16 rounds the odd ones above 256)
        for name, _, kind, what in fwd16:
            want = ref[what] if isinstance(what, str) else ref["acts"][what]
            rnd = obrnn.round_f16 if kind == "float16" else obrnn.round_bf16
            dim = D if what == 0 else H
            X = sh16[name]
            assert X.shape[0] == sum(Ts) and X.shape[1] % 32 == 0 and X.shape[1] >= dim
            assert not X[:, dim:].any(), "%s: padding columns of %s are not zero" % (c.id, name)
            for b, (g, r) in enumerate(zip(_per_utt(X, rows, dim), want)):
                np.testing.assert_array_equal(np.float32(g), np.float32(rnd(r)), err_msg="%s %s utterance %d" % (c.id, name, b))
    np.testing.assert_array_equal(skips, ref["skips"])
    assert not skips.any()
    np.testing.assert_allclose(costs, ref["costs"], rtol=1e-5)

    if c.id == TWICE:
        assert fp32
        net.costAndGradBatch(case.datas, case.labs)
        again = _device_grads(net, NL)
        for (name, a), (_, b_) in zip(en.grad_tensors(grads), en.grad_tensors(again)):
            np.testing.assert_array_equal(a, b_, err_msg=name)
        np.testing.assert_array_equal(d1, net.debugBuffer(200))
    del net
    st = case.stats
    shares = " | ".join("%s open %.3f zero %.3f clipped %.3f pre==0 %d pre==max %d"
                        % (d, st[d]["open"], st[d]["zero"], st[d]["clipped"], st[d]["pre_eq_0"], st[d]["pre_eq_max"]) for d in "FB")
    if not fp32:
        # ---- backward, fp16 operands: against the float64 rounding model, bounded by the float32 rounding model's own error
        mixed = en.rounding_of(c)
        m64 = en.reference(case, mixed=mixed)
        e_ref = en.mixed_e_ref(c.H, c.B, c.NL, c.TL, c.Tmax, mixed.rec16)
        for k in en.SHADOWS:
            assert not sh16[k][:, H:].any(), "%s: padding columns of the bfloat16 shadow %s are not zero" % (c.id, k)
        dev = {"grads": grads, "dF": _per_utt(dF, rows, H), "dB": _per_utt(dBk, rows, H),
               "shadows": {k: _per_utt(sh16[k], rows, H) for k in en.SHADOWS}}
        st = en.mixed_stats(dev, m64, case.max_act)
        rel = {k: v for k, v in st.items() if k.startswith(("fro:", "row:"))}
        worst = max(rel, key=lambda k: rel[k] / max(e_ref[k], en.FLOOR))
        vs_exact = [(name, en.rel_fro(g, r)) for (name, g), (_, r) in zip(en.grad_tensors(grads), en.grad_tensors(ref["grads"]))]
        _note("exact %-30s frames %4d  %s  fp16 backward: worst ratio %.2f (%s: e_dev %.2e e_ref %.2e); shares %s; zeros %s; vs exact max %.1e; "
              "e_dev/e_ref %s" % (c.id, sum(Ts), shares, rel[worst] / max(e_ref[worst], en.FLOOR), worst[4:], rel[worst], e_ref[worst],
                                  " ".join("%s %.1e" % (k, st["share:" + k]) for k in en.SHADOWS),
                                  " ".join("%d" % st[k] for k in ("open:dF", "open:dB", "dirty:d1")), max(e for _, e in vs_exact),
                                  " ".join("%s %.1e/%.1e" % (k[4:], rel[k], e_ref[k]) for k in rel)))
        assert en.mixed_violations(st, e_ref, MARGIN) == []
        for name, e in vs_exact:
            assert e <= TOL_FP16_EXACT, (name, e)
        return

    # ---- backward: per frame, per tensor, against the float32 restatement's own error
    ref32 = en.reference(case, dtype=np.float32)
    rho_32, dirty_32 = en.row_errors(ref32["d1"], ref["d1"])
    rho_dev, dirty = en.row_errors(_per_utt(d1, rows, H), ref["d1"])
    assert dirty_32 == 0 and rho_32 > 0
    worst = ("d1", rho_dev / rho_32)
    tens = []
    for (name, g), (_, r64), (_, r32) in zip(en.grad_tensors(grads), en.grad_tensors(ref["grads"]), en.grad_tensors(ref32["grads"])):
        e_dev, e_32 = en.rel_fro(g, r64), en.rel_fro(r32, r64)
        tens.append((name, e_dev, e_32))
        if e_32 > 0 and e_dev / e_32 > worst[1]:
            worst = (name, e_dev / e_32)
    _note("exact %-30s frames %4d  %s  rho_dev %.2e rho_32 %.2e ratio %.2f; worst ratio %.2f (%s); tensors %s"
          % (c.id, sum(Ts), shares, rho_dev, rho_32, rho_dev / rho_32, worst[1], worst[0],
             " ".join("%s %.1e/%.1e" % t for t in tens)))
    assert dirty == 0, "%d frames of delta_1 are exactly zero in the reference and not on the device" % dirty
    assert rho_dev <= MARGIN * rho_32, (rho_dev, rho_32)
    assert rho_dev <= TOL_MASKED, rho_dev
    for name, e_dev, e_32 in tens:
        assert e_dev <= MARGIN * e_32, (name, e_dev, e_32)
        assert e_dev <= TOL_MASKED, (name, e_dev)
