"""float64 NumPy restatements of every kernel of stanford-ctc_amd/csrc/elementwise.hip, and the case tables of
tests/test_gpu_elementwise.py (the device) and tests/test_elementwise_model_cpu.py (exactness and liveness on the CPU).

Optimizer entries (public ABI): sctc_axpy, sctc_scale, sctc_sumsq, sctc_sumsq_reg, sctc_nesterov_step,
sctc_nesterov_step_reg.  Their cases live on a grid on which fp32 is exact in any order, fused or not:

    w, v, g                                    multiples of 2^-4 in [-64, 64]
    mom, alpha, grad_scale, reg, max_gnorm     powers of two
    *sumsq                                     written by the test, a power of four (sqrt and clip ratio exact)

so the device must agree BIT FOR BIT.  `Arith` evaluates the same expressions exactly ("f64", asserting that every
intermediate equals its own float32 cast), with every operation rounded to float32 ("f32"), or with each
multiply-add rounded once ("fma"); the CPU test proves the three agree for every case.

Internal launchers (through tools/diag/elementwise_entry.hip): gather_rows, scatter_rows, add, cvt16, add16,
transpose_bf16, gather_rows16.  They move or round values, so their models are exact for ANY input; the 16-bit
roundings work on bit patterns (float16 through NumPy's astype, bfloat16 by its own nearest-even; NaN stays NaN,
which oracle.brnn.round_bf16 does not guarantee -- compare NaN outputs with `same16` / `same32`).

`mut` names one deliberate mistake (MUTATIONS); the CPU test proves that the tables notice each of them.

The edges of the tables come from the launch code: grid_for caps the grid at 2048 blocks of 256 threads (one pass =
524288 elements, or 2097152 floats for the float4 kernels add / cvt16 / add16), launch_sumsq at 1024 blocks (262144),
the row kernels put four rows in a block, the transpose works on 32 x 32 tiles, MAX_NOREG_RANGES is 128."""
from types import SimpleNamespace

import numpy as np

PASS = 2048 * 256           # elements one pass of a grid_for() grid covers
SS_PASS = 1024 * 256        # the same for the two sum-of-squares entries (SS_BLOCKS)
F4_PASS = 4 * PASS          # floats one pass of the float4 kernels covers
MAX_NOREG_RANGES = 128
SENT = np.float32(-12345.0)         # guard / "never written" fill of fp32 buffers
SENT16 = np.uint16(0xA5C3)          # ... of 16-bit buffers (a finite negative value in both formats)

MUTATIONS = (
    "skip_last_partial_block",      # the elements of the last, partial block are never visited
    "first_pass_only",              # the grid-stride loop never wraps
    "range_beg_exclusive", "range_end_inclusive",       # a no-L2 range edge off by one
    "parity_inverted",              # the L2 term applied INSIDE the ranges only
    "l2_at_w",                      # the L2 term taken at w instead of w + mom * v
    "v_updated_before_l2",          # the velocity stored after the data term, then read for the L2 term
    "grad_scale_twice", "grad_scale_dropped",
    "clip_rule_swapped",            # the clip rule of one Nesterov kernel used in the other
    # "vel null ignored in sumsq_reg", read as: vel is given but the L2 term is taken at w, as if it were null.  The
    # other reading (vel null, yet dereferenced) is a fault on a device, not a wrong number; the vel-null cases
    # cover that direction.
    "vel_ignored",
    "f16_truncates", "bf16_truncates", "f16_ties_away", "bf16_ties_away",
    "add16_input_shadows_swapped",
    "transpose_untransposed",       # dst[r][c] written instead of dst[c][r]
    "gather_pads_to_64_lanes",      # zero padding only up to cols rounded up to 64, not to ldd
    "gather_padding_unwritten",
)


def f32(x):
    return np.float64(np.float32(x))


# ------------------------------------------------------------------------------------------ 16-bit roundings (bits)

def f16_bits(x, mode=None):
    """float16 bit patterns of float32 x, round-to-nearest-even; mode "trunc" / "ties_away": the mutants"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = x.astype(np.float16)
    bits = h.view(np.uint16).copy()
    if mode is None:
        return bits
    fin = np.isfinite(x)
    with np.errstate(invalid="ignore"):
        ax = np.abs(x.astype(np.float64))
        up =fin & (np.abs(h.astype(np.float64)) > ax)          # nearest-even went away from zero (inf included)
    lo_bits = bits.copy()
    lo_bits[up] -= 1                                            # sign-magnitude: one step toward zero
    if mode == "trunc":
        return lo_bits
    assert mode == "ties_away", mode
    lo = np.abs(lo_bits.view(np.float16).astype(np.float64))
    hi_bits = (lo_bits + np.uint16(1)).astype(np.uint16)
    with np.errstate(invalid="ignore"):
        hi = np.abs(hi_bits.view(np.float16).astype(np.float64))
    hi[(hi_bits & 0x7FFF) == 0x7C00] = 65536.0                  # the step after 65504, were the exponent unbounded
    out = bits.copy()
    with np.errstate(invalid="ignore"):
        tie = fin & (ax != lo) & (ax - lo == hi - ax)
    out[tie] = hi_bits[tie]
    return out


def bf16_bits(x, mode=None):
    """bfloat16 bit patterns of float32 x, round-to-nearest-even on the bit pattern; a NaN stays a NaN (0x7FC0 here:
    compare with same16)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    if mode == "trunc":
        r = u >> 16
    elif mode == "ties_away":
        r = (u + 0x8000) >> 16
    else:
        assert mode is None, mode
        r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    r = r.astype(np.uint16)
    r[np.isnan(x)] = 0x7FC0
    return r


def isnan16(bits, kind):
    bits = np.asarray(bits, dtype=np.uint16)
    if kind == "f16":
        return ((bits & 0x7C00) == 0x7C00) & ((bits & 0x03FF) != 0)
    assert kind == "bf16", kind
    return ((bits & 0x7F80) == 0x7F80) & ((bits & 0x007F) != 0)


def same16(got, want, kind):
    """elementwise: equal bit patterns, or both NaN"""
    return (got == want) | (isnan16(got, kind) & isnan16(want, kind))


def same32(got, want):
    """elementwise on float32 images: equal BITS (so -0 differs from +0), or both NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def _u32(*patterns):
    return np.array(patterns, dtype=np.uint32).view(np.float32)


def shadow_specials():
    """float32 inputs at which a 16-bit rounding can go wrong, each also negated"""
    nx = np.nextafter
    one = np.float32(1.0)
    pos = np.concatenate([
        np.array([0.0, np.inf, 3.4028234663852886e38], dtype=np.float32),
        # float16: 2049 / 2051 are ties (spacing 2 above 2048): down to 2048, up to 2052; 65504 is the largest finite;
        # below 65520 -> 65504, 65520 (the tie) -> inf; 2^-14 the smallest normal, 2^-24 the smallest denormal;
        # 2^-25 is the tie with zero (-> 0), the next float32 above it -> 2^-24; 3 * 2^-25 ties to 2^-23 (even)
        np.array([2049.0, 2051.0, 65504.0, nx(np.float32(65520.0), one), 65520.0, 2.0 ** -14, 2.0 ** -24,
                  2.0 ** -25, nx(np.float32(2.0 ** -25), one), 3 * 2.0 ** -25, 2.0 ** -26], dtype=np.float32),
        # bfloat16 (8 significant bits): 1 + 2^-8 ties down to 1, 1 + 3 * 2^-8 ties up to 1 + 2^-6; 0x7F7F7FFF is the
        # largest value that stays finite, 0x7F7F8000 (the tie) and everything above it round to inf
        np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20], dtype=np.float32),
        _u32(0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001),
        # fp32 denormals: IEEE nearest-even to bfloat16 denormals (0x8000 ties to 0, 0x18000 ties to 2), zero in float16
        _u32(0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x00014000, 0x007FFFFF, 0x00800000),
    ])
    nans = _u32(0x7FC00000, 0x7F800001, 0xFFC00000, 0x7FBFFFFF)         # quiet, small payload, negative, signalling
    return np.concatenate([pos, -pos, nans]).astype(np.float32)


def shadow_data(n, seed):
    """n float32 values that need rounding in both formats (24 random mantissa bits, exponents -8..8), with the
    specials spread over the buffer: its start, its end (the last partial block) and the middle (every pass)"""
    rs = np.random.RandomState(seed)
    m = rs.randint(0, 1 << 23, size=n).astype(np.uint32)
    e = rs.randint(127 - 8, 127 + 9, size=n).astype(np.uint32)
    s = rs.randint(0, 2, size=n).astype(np.uint32)
    x = ((s << 31) | (e << 23) | m).view(np.float32)
    sp = shadow_specials()
    k = len(sp)
    if n >= k:
        x[:k] = sp
        x[n - k:] = sp[::-1]
    else:
        x[:] = sp[:n]
    for start in range(F4_PASS - k // 2, n - k, F4_PASS):      # across every pass boundary of the float4 kernels
        x[start:start + k] = sp
    return x


# ------------------------------------------------------------------------------------------ arithmetic

class Arith(object):
    """mode "f64": exact double arithmetic; with exact=True every result must equal its own float32 cast (the grid
    property).  "f32": every operation rounded to float32.  "fma": a * b + c rounded to float32 once."""

    def __init__(self, mode="f64", exact=False):
        assert mode in ("f64", "f32", "fma"), mode
        self.mode, self.exact = mode, exact

    def r(self, x):
        x = np.asarray(x, dtype=np.float64)
        y = x.astype(np.float32).astype(np.float64)
        if self.mode == "f64":
            if self.exact:
                assert np.array_equal(x, y), "an intermediate is not a float32: the case is off the exact grid"
            return x
        return y

    def mul(self, a, b):
        return self.r(np.asarray(a, dtype=np.float64) * b)

    def add(self, a, b):
        return self.r(np.asarray(a, dtype=np.float64) + b)

    def fma(self, a, b, c):
        if self.mode == "fma":
            return self.r(np.asarray(a, dtype=np.float64) * b + c)      # the product of two float32 is exact in float64
        return self.add(self.mul(a, b), c)


def visited(n, one_pass, mut, per_block=256):
    """which of n elements a (mutated) grid-stride loop visits"""
    vis = np.ones(n, dtype=bool)
    if mut == "skip_last_partial_block" and n % per_block:
        vis[n // per_block * per_block:] = False
    if mut == "first_pass_only":
        vis[one_pass:] = False
    return vis


def inside_ranges(n, ranges, mut=None):
    """bool[n]: element lies in one of the [beg, end) ranges (flat int64 list, ascending, disjoint)"""
    ins = np.zeros(n, dtype=bool)
    for beg, end in np.asarray(ranges, dtype=np.int64).reshape(-1, 2).tolist():
        if mut == "range_beg_exclusive":
            beg += 1
        if mut == "range_end_inclusive" and end > beg:
            end += 1
        ins[max(0, beg):max(0, min(n, end))] = True
    return ~ins if mut == "parity_inverted" else ins


def clip_alpha(alpha, max_gnorm, grad_scale, S, rule):
    """the learning rate after the global-norm clip.  rule "plain" (nesterov_kernel): gnorm = sqrt(S) * grad_scale;
    "reg" (nesterov_reg_kernel): gnorm = sqrt(S), its sum already holds the scaled effective gradient.  In double, the
    result cast to float32, like the kernels."""
    a = f32(alpha)
    if S is None:
        return a
    gnorm = np.sqrt(np.float64(S)) * (f32(grad_scale) if rule == "plain" else 1.0)
    if gnorm > f32(max_gnorm):
        a = f32(a * (f32(max_gnorm) / gnorm))
    return a


# ------------------------------------------------------------------------------------------ optimizer models

def axpy(ar, y, x, alpha, mut=None):
    out = ar.fma(f32(alpha), x, y)
    return np.where(visited(len(y), PASS, mut), out, y)


def scale(ar, x, alpha, mut=None):
    return np.where(visited(len(x), PASS, mut), ar.mul(f32(alpha), x), x)


def exact_sumsq(t):
    """sum t^2 in integers: t are multiples of 2^-20 here, the sum must stay below 2^53 units to be a double"""
    k = np.asarray(t, dtype=np.float64) * 2.0 ** 20
    ki = k.astype(np.int64)
    assert np.array_equal(ki.astype(np.float64), k), "not on the 2^-20 grid"
    # two limbs of 2^16 keep every partial sum far below 2^63
    hi, lo = ki >> 16, ki & 0xFFFF
    total = (int(np.sum(hi * hi)) << 32) + (int(np.sum(hi * lo)) << 17) + int(np.sum(lo * lo))
    assert total < 2 ** 53 or total % (1 << (total.bit_length() - 53)) == 0, "the exact sum is not a double"
    return float(total) / 2.0 ** 40


def sumsq(x, mut=None, exact=True):
    x = np.asarray(x, dtype=np.float64)[visited(len(x), SS_PASS, mut)]
    return exact_sumsq(x) if exact else float(np.sum(x * x))


def sumsq_reg(ar, g, w, vel, mom, grad_scale, reg, ranges, mut=None, exact=True):
    """sum (grad_scale * g + reg_i * (w + mom * vel))^2, each term formed in float32, squared and summed in double;
    vel None: the L2 term at w"""
    n = len(g)
    regi = np.where(inside_ranges(n, ranges, mut), 0.0, f32(reg))
    wl = w if (vel is None or mut == "vel_ignored") else ar.fma(f32(mom), vel, w)
    gs = f32(grad_scale)
    gsg = g if mut == "grad_scale_dropped" else ar.mul(gs, g)
    if mut == "grad_scale_twice":
        gsg = ar.mul(gs, gsg)
    t = ar.fma(regi, wl, gsg)[visited(n, SS_PASS, mut)]
    return exact_sumsq(t) if exact else float(np.sum(t * t))


def nesterov(ar, w, v, g, mom, alpha, max_gnorm, grad_scale, S, mut=None):
    """v' = mom * v - (alph * grad_scale) * g ;  w' = w + v'   -> (w', v')"""
    alph = clip_alpha(alpha, max_gnorm, grad_scale, S, "reg" if mut == "clip_rule_swapped" else "plain")
    gs = f32(grad_scale)
    ga = alph if mut == "grad_scale_dropped" else ar.mul(alph, gs)
    if mut == "grad_scale_twice":
        ga = ar.mul(ga, gs)
    nv = ar.fma(-ga, g, ar.mul(f32(mom), v))
    nw = ar.add(w, nv)
    vis = visited(len(w), PASS, mut)
    return np.where(vis, nw, w), np.where(vis, nv, v)


def nesterov_reg(ar, w, v, g, mom, alpha, max_gnorm, grad_scale, reg, ranges, S, mut=None):
    """e = grad_scale * g + reg_i * (w + mom * v) ;  v' = mom * v - alph * e ;  w' = w + v'   -> (w', v')"""
    n = len(w)
    alph = clip_alpha(alpha, max_gnorm, grad_scale, S, "plain" if mut == "clip_rule_swapped" else "reg")
    gs, m = f32(grad_scale), f32(mom)
    regi = np.where(inside_ranges(n, ranges, mut), 0.0, f32(reg))
    gsg = g if mut == "grad_scale_dropped" else ar.mul(gs, g)
    if mut == "grad_scale_twice":
        gsg = ar.mul(gs, gsg)
    if mut == "v_updated_before_l2":
        v1 = ar.fma(-alph, gsg, ar.mul(m, v))
        nv = ar.fma(-alph, ar.mul(regi, ar.fma(m, v1, w)), v1)
    else:
        look = w if mut == "l2_at_w" else ar.fma(m, v, w)
        e = ar.fma(regi, look, gsg)
        nv = ar.fma(-alph, e, ar.mul(m, v))
    nw = ar.add(w, nv)
    vis = visited(n, PASS, mut)
    return np.where(vis, nw, w), np.where(vis, nv, v)


# ------------------------------------------------------------------------------------------ layout / shadow models
# every model takes the images of the buffers it may write (flat payloads, without the test's guards) and returns new ones

def ceil64(c):
    return (int(c) + 63) // 64 * 64


def add(out0, a, b, n, mut=None):
    out = np.array(out0, dtype=np.float32)
    vis = visited(n, F4_PASS, mut, per_block=1024)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (a[:n].astype(np.float64) + b[:n].astype(np.float64)).astype(np.float32)
    out[:n][vis] = s[vis]
    return out


def _rounders(mut):
    def fa(x):
        return f16_bits(x, {"f16_truncates": "trunc", "f16_ties_away": "ties_away"}.get(mut))

    def fb(x):
        return bf16_bits(x, {"bf16_truncates": "trunc", "bf16_ties_away": "ties_away"}.get(mut))
    return fa, fb


def cvt16(img, src, n, mut=None):
    """img: dict f16 / bf16 -> initial image or None (null pointer); returns the images after the launch"""
    fa, fb = _rounders(mut)
    vis = visited(n, F4_PASS, mut, per_block=1024)
    out = {}
    for k, fn in (("f16", fa), ("bf16", fb)):
        out[k] = None
        if img.get(k) is not None:
            out[k] = np.array(img[k], dtype=np.uint16)
            out[k][:n][vis] = fn(src[:n])[vis]
    return out


def add16(img, a, b, n, mut=None):
    """img: dict out / o_f16 / o_bf16 / a_bf16 / b_bf16 -> initial image or None.  The shadows of the sum are the
    roundings of the float32 sum; a_bf16 / b_bf16 those of the inputs themselves."""
    fa, fb = _rounders(mut)
    vis = visited(n, F4_PASS, mut, per_block=1024)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (a[:n].astype(np.float64) + b[:n].astype(np.float64)).astype(np.float32)
    xa, xb = (b, a) if mut == "add16_input_shadows_swapped" else (a, b)
    vals = {"out": lambda: s, "o_f16": lambda: fa(s), "o_bf16": lambda: fb(s), "a_bf16": lambda: fb(xa[:n]),
            "b_bf16": lambda: fb(xb[:n])}
    out = {}
    for k, fn in vals.items():
        out[k] = None
        if img.get(k) is not None:
            out[k] = np.array(img[k])
            out[k][:n][vis] = fn()[vis]
    return out


def gather_rows16(img, ldd, src, lds, idx, rows, cols, mut=None):
    """img: dict dst / f16 / bf16 -> initial image or None (dst is never null).  dst[r][0..ldd) = src[idx[r]][0..cols),
    zero from cols to ldd, in fp32 and in each shadow present"""
    fa, fb = _rounders(mut)
    S = np.asarray(src, dtype=np.float32)
    rowsel = np.asarray(idx[:rows], dtype=np.int64)[:, None] * lds + np.arange(cols)[None, :]
    vals = S[rowsel]                                                    # rows x cols
    pad_to = ldd
    if mut == "gather_pads_to_64_lanes":
        pad_to = min(ldd, ceil64(cols))
    if mut == "gather_padding_unwritten":
        pad_to = cols
    out = {}
    for k, fn in (("dst", lambda x: x), ("f16", fa), ("bf16", fb)):
        out[k] = None
        if img.get(k) is not None:
            o = np.array(img[k])
            D = o[:rows * ldd].reshape(rows, ldd)
            D[:, cols:pad_to] = fn(np.zeros(1, dtype=np.float32))[0]
            D[:, :cols] = fn(vals.reshape(-1)).reshape(rows, cols)
            out[k] = o
    return out


def gather_rows(dst0, ldd, src, lds, idx, rows, cols, mut=None):
    return gather_rows16({"dst": dst0}, ldd, src, lds, idx, rows, cols, mut)["dst"]


def scatter_rows(dst0, ldd, src, lds, idx, rows, cols):
    """dst[idx[r]][0..cols) = src[r][0..cols); nothing else is written"""
    o = np.array(dst0, dtype=np.float32)
    ii = np.asarray(idx[:rows], dtype=np.int64)[:, None] * ldd + np.arange(cols)[None, :]
    si = np.arange(rows)[:, None] * lds + np.arange(cols)[None, :]
    o[ii] = np.asarray(src, dtype=np.float32)[si]
    return o


def transpose_bf16(dst0, ldd, src, lds, rows, cols, mut=None):
    """dst[c][r] = bf16(src[r][c]) for r < rows, c < cols; nothing else is written"""
    _, fb = _rounders(mut)
    o = np.array(dst0, dtype=np.uint16)
    si = np.arange(rows)[:, None] * lds + np.arange(cols)[None, :]
    vals = fb(np.asarray(src, dtype=np.float32)[si].reshape(-1)).reshape(rows, cols)
    if mut == "transpose_untransposed":
        di = np.arange(rows)[:, None] * ldd + np.arange(cols)[None, :]
        ok = di < len(o)
        o[di[ok]] = vals[ok]
        return o
    di = np.arange(cols)[:, None] * ldd + np.arange(rows)[None, :]
    o[di] = vals.T
    return o


# ------------------------------------------------------------------------------------------ optimizer case table

OPT_NS = (0, 1, 255, 256, 257, PASS - 1, PASS, PASS + 1, 3 * PASS + 77)         # block edge; one pass -+ 1; wraps + tail
SS_NS = (1, 255, 257, SS_PASS - 1, SS_PASS, SS_PASS + 1, 5 * SS_PASS + 3)       # the 1024-block cap -+ 1; many wraps
S_CLIP = 2.0 ** 22          # sqrt = 2048


def production_layout(D=483, H=1824, NL=5, A=33):
    """(n, no-L2 ranges) of the cfg-3 network of bench.py (inputDim 483, 5 x 1824, 33 symbols, temporal layer): the flat
    parameter buffer as csrc/brnn_engine.hip lays it out -- W_l [pad32(out)][ceil64(in)] then b_l [pad32(out)], then
    Wf, Wb -- with the bias ranges as NNet.noreg_ranges forms them (offset, offset + padded rows)"""
    import cudamat as cm
    sizes = [D] + [H] * NL + [A]
    off, ranges = 0, []
    for n_in, n_out in zip(sizes[:-1], sizes[1:]):
        rows_p, ld = cm.padded_layout(n_out, n_in)
        off += rows_p * ld
        rb, _ = cm.padded_layout(n_out, 1)
        ranges += [off, off + rb]
        off += rb
    rows_p, ld = cm.padded_layout(H, H)
    off += 2 * rows_p * ld
    return off, np.array(ranges, dtype=np.int64)


def edge_ranges(n):
    """ranges with every edge kind, for n >= 512: starting at 0, an empty one in the middle, single elements, two
    adjacent pairs, one ending at n; plus one that straddles the end of the first pass when n reaches it"""
    r = [0, 5, 9, 9, 20, 21, 21, 22, 100, 300, 300, 301]
    for p in (SS_PASS, PASS):
        if n > p + 16:
            r += [p - 3, p + 5]
    r += [n - 7, n]
    return np.array(r, dtype=np.int64)


def sweep_ranges(n):
    if n >= 512:
        return edge_ranges(n)
    if n >= 4:
        return np.array([0, 1, n // 2, n // 2, n - 1, n], dtype=np.int64)
    return np.array([0, 1] if n >= 1 else [], dtype=np.int64)


def many_ranges(n, k=MAX_NOREG_RANGES):
    """k ranges of 1..3 elements, evenly spread"""
    step = n // k
    assert step >= 4
    r = []
    for i in range(k):
        r += [i * step + 1, i * step + 2 + i % 3]
    return np.array(r, dtype=np.int64)


def _opt(kernel, name, n, note, **kw):
    d = dict(kernel=kernel, name="%s-%s" % (kernel, name), n=n, note=note, off=0, mom=0.5, alpha=2.0 ** -3,
             max_gnorm=128.0, grad_scale=0.25, reg=0.25, S=S_CLIP, ranges=np.zeros(0, dtype=np.int64), vel=True,
             production=False)
    unknown = set(kw) - set(d)
    assert not unknown, unknown
    d.update(kw)
    return SimpleNamespace(**d)


def optimizer_cases():
    cs = []
    for k in ("axpy", "scale", "nesterov", "nesterov_reg"):
        for n in OPT_NS:
            cs.append(_opt(k, "n%d" % n, n, "grid_for: 256 per block, 2048 blocks = %d per pass" % PASS,
                           ranges=sweep_ranges(n) if k == "nesterov_reg" else np.zeros(0, dtype=np.int64)))
        cs.append(_opt(k, "misaligned", 1027, "every pointer offset by one float: 4-byte alignment only", off=1,
                       ranges=sweep_ranges(1027) if k == "nesterov_reg" else np.zeros(0, dtype=np.int64)))
    # the clip: sqrt(S) = 2048.  nesterov: gnorm = 2048 / 4 = 512 > 128, alph = alpha / 4 (the other rule: / 16).
    # Not taken: nesterov sqrt(2^16) / 4 = 64 <= 128 (the other rule takes it: 256); nesterov_reg sqrt(2^12) = 64 with
    # grad_scale 4 (the other rule takes it: 256).
    cs.append(_opt("nesterov", "clip-taken", 1000, "gnorm = sqrt(S) * grad_scale > max_gnorm"))
    cs.append(_opt("nesterov", "clip-not-taken", 1000, "sqrt(S) > max_gnorm >= sqrt(S) * grad_scale", S=2.0 ** 16))
    cs.append(_opt("nesterov", "clip-null", 1000, "sumsq_dev null: no clip", S=None))
    rr = edge_ranges(1000)
    cs.append(_opt("nesterov_reg", "clip-taken", 1000, "gnorm = sqrt(S) > max_gnorm", ranges=rr))
    cs.append(_opt("nesterov_reg", "clip-not-taken", 1000, "sqrt(S) * grad_scale > max_gnorm >= sqrt(S)", S=2.0 ** 12,
                   grad_scale=4.0, ranges=rr))
    cs.append(_opt("nesterov_reg", "clip-null", 1000, "sumsq_dev null: no clip", S=None, ranges=rr))
    for k in ("sumsq", "sumsq_reg"):
        for n in SS_NS:
            cs.append(_opt(k, "n%d" % n, n, "launch_sumsq: 1024 blocks = %d per pass" % SS_PASS,
                           ranges=sweep_ranges(n) if k == "sumsq_reg" else np.zeros(0, dtype=np.int64)))
        cs.append(_opt(k, "misaligned", 1027, "every float pointer offset by one float", off=1,
                       ranges=sweep_ranges(1027) if k == "sumsq_reg" else np.zeros(0, dtype=np.int64)))
    cs.append(_opt("sumsq_reg", "vel-null", 4099, "vel null: the L2 term at w", vel=False, ranges=edge_ranges(4099)))
    # the no-L2 ranges (reg_at's binary search; MAX_NOREG_RANGES = 128)
    pn, pr = production_layout()
    for k in ("sumsq_reg", "nesterov_reg"):
        cs.append(_opt(k, "ranges-0", 4099, "no range: L2 everywhere"))
        cs.append(_opt(k, "ranges-1", 4099, "one range", ranges=np.array([1366, 2049], dtype=np.int64)))
        cs.append(_opt(k, "ranges-128", 4099, "MAX_NOREG_RANGES ranges", ranges=many_ranges(4099)))
        cs.append(_opt(k, "ranges-edges", 4099, "at 0, empty, single, adjacent, at n", ranges=edge_ranges(4099)))
        cs.append(_opt(k, "production", pn, "the cfg-3 flat buffer, bias ranges of NNet.noreg_ranges", ranges=pr,
                       production=True))
    return cs


def grid_values(rs, n):
    return (rs.randint(-1024, 1025, size=n) / 16.0).astype(np.float32)


def optimizer_data(c, real=False):
    """host inputs of case c: float32 w, v, g (x, y for axpy / scale / sumsq); real: standard normal instead of the grid"""
    import zlib
    rs = np.random.RandomState(zlib.crc32(c.name.encode()) & 0x7FFFFFFF)
    gen = (lambda: rs.randn(c.n).astype(np.float32)) if real else (lambda: grid_values(rs, c.n))
    return SimpleNamespace(w=gen(), v=gen(), g=gen())


def optimizer_model(c, d, mode="f64", exact=True, mut=None):
    """-> dict of what case c leaves behind: w / v images (float64 values), or "out" (the sum)"""
    exact = exact and mut is None           # a mutant may leave the grid
    ar = Arith(mode, exact and mode == "f64")
    w, v, g = (x.astype(np.float64) for x in (d.w, d.v, d.g))
    k = c.kernel
    if k == "axpy":         # y = w, x = g
        return {"w": axpy(ar, w, g, c.alpha, mut)}
    if k == "scale":
        return {"w": scale(ar, w, c.alpha, mut)}
    if k == "sumsq":
        return {"out": sumsq(g, mut, exact)}
    if k == "sumsq_reg":
        return {"out": sumsq_reg(ar, g, w, v if c.vel else None, c.mom, c.grad_scale, c.reg, c.ranges, mut, exact)}
    if k == "nesterov":
        nw, nv = nesterov(ar, w, v, g, c.mom, c.alpha, c.max_gnorm, c.grad_scale, c.S, mut)
        return {"w": nw, "v": nv}
    assert k == "nesterov_reg", k
    nw, nv = nesterov_reg(ar, w, v, g, c.mom, c.alpha, c.max_gnorm, c.grad_scale, c.reg, c.ranges, c.S, mut)
    return {"w": nw, "v": nv}


OPT_MUTATIONS = {
    "axpy": ("skip_last_partial_block", "first_pass_only"),
    "scale": ("skip_last_partial_block", "first_pass_only"),
    "sumsq": ("skip_last_partial_block", "first_pass_only"),
    "nesterov": ("skip_last_partial_block", "first_pass_only", "grad_scale_twice", "grad_scale_dropped",
                 "clip_rule_swapped"),
    "sumsq_reg": ("skip_last_partial_block", "first_pass_only", "range_beg_exclusive", "range_end_inclusive",
                  "parity_inverted", "grad_scale_twice", "grad_scale_dropped", "vel_ignored"),
    "nesterov_reg": ("skip_last_partial_block", "first_pass_only", "range_beg_exclusive", "range_end_inclusive",
                     "parity_inverted", "l2_at_w", "v_updated_before_l2", "grad_scale_twice", "grad_scale_dropped",
                     "clip_rule_swapped"),
}

# rejected range lists: (name, n_ranges, flat list or None) -- each gives the argument error, nothing written
BAD_RANGES = (
    ("129-ranges", 129, np.arange(258, dtype=np.int64) * 4),
    ("descending", 2, np.array([10, 20, 15, 30], dtype=np.int64)),
    ("null-list", 1, None),
)


# ------------------------------------------------------------------------------------------ launcher case tables

F4_NS = (4, 1020, 1024, 1028, F4_PASS - 4, F4_PASS, F4_PASS + 4, 2 * F4_PASS + 12)      # block edge; one pass -+ a float4
ADD16_OUTPUTS = ("out", "o_f16", "o_bf16", "a_bf16", "b_bf16")
ADD16_COMBOS = tuple((k,) for k in ADD16_OUTPUTS) + (
    ADD16_OUTPUTS,
    ("o_f16", "o_bf16", "a_bf16", "b_bf16"),    # brnn_engine.hip, forward sum of the two directions while training: out null
    ("o_bf16", "a_bf16", "b_bf16"),             # brnn_engine.hip, backward sum of the two delta matrices: out and o_f16 null
)
ROWS = (1, 3, 4, 5, 1023, 1025)         # four rows per block; one grid edge beyond 1024
COLS = (1, 63, 64, 65, 615)             # one wave of 64 lanes per row
RAGGED = (1, 31, 33, 95)
TRANSPOSE_PADDED = ((32, 32), (96, 64), (64, 1824), (1824, 1824))      # (rows = padded outputs, cols = padded H)


def add16_inputs(n, seed):
    """a, b whose sum meets the specials: a = the shadow data with b = -0 there (x + -0 = x, for -0 and +0 too), random
    elsewhere; plus inf + -inf, max + max and two denormals"""
    a = shadow_data(n, seed)
    rs = np.random.RandomState(seed + 1)
    m = rs.randint(0, 1 << 23, size=n).astype(np.uint32)
    e = rs.randint(127 - 8, 127 + 9, size=n).astype(np.uint32)
    b = (((m & 1) << 31) | (e << 23) | m).view(np.float32).copy()
    sp = shadow_specials()
    special = np.isin(a.view(np.uint32), sp.view(np.uint32))
    b[special] = -0.0
    if n >= 4 * len(sp):
        i = 2 * len(sp)
        a[i:i + 4] = _u32(0x7F800000, 0x7F7FFFFF, 0x00000003, 0x00400000)
        b[i:i + 4] = _u32(0xFF800000, 0x7F7FFFFF, 0x00000005, 0x00400000)
    return a, b


def row_case(rows, cols, seed, extra_ld=0, scatter=False):
    """one gather / scatter shape: ldd = ceil64(cols) (+ extra_ld), lds = cols + 3; the source of a gather has two
    rows more than `rows`, with idx drawing from all of them (duplicates, out of order); the destination of a scatter
    two rows more, idx a permutation"""
    rs = np.random.RandomState(seed)
    c = SimpleNamespace(rows=rows, cols=cols, name="r%d-c%d%s" % (rows, cols, "-ld+%d" % extra_ld if extra_ld else ""))
    n_other = rows + 2
    if scatter:
        c.ldd, c.lds = ceil64(cols) + extra_ld, cols + 3
        c.idx = rs.permutation(n_other)[:rows].astype(np.int32)
        c.src = grid_values(rs, rows * c.lds)
        c.dst_elems = n_other * c.ldd
    else:
        c.ldd, c.lds = ceil64(cols) + extra_ld, cols + 3
        c.idx = rs.randint(0, n_other, size=rows).astype(np.int32)
        if rows >= 2:
            c.idx[-1] = c.idx[0]                        # a duplicate for certain
        src = shadow_data(n_other * c.lds, seed).reshape(n_other, c.lds)
        src[:, cols:] = np.nan                          # never read: would show in the zero padding
        c.src = src.reshape(-1)
        c.dst_elems = rows * c.ldd
    return c


def row_cases(scatter=False):
    cs = [row_case(r, c, 1000 * r + c, scatter=scatter) for r in ROWS for c in COLS]
    if not scatter:     # ldd beyond the 64-lane round-up of cols: every stride of the padding loop
        cs += [row_case(5, 65, 77, extra_ld=64), row_case(3, 1, 78, extra_ld=128)]
    return cs


def transpose_cases():
    """(rows, cols, lds, ldd, src): the engine's padded shapes with its leading dimensions (ceil64 of the extent), and
    ragged ones with both leading dimensions larger than the extent"""
    cs = []
    for rows, cols in TRANSPOSE_PADDED:
        cs.append(SimpleNamespace(rows=rows, cols=cols, lds=ceil64(cols), ldd=ceil64(rows)))
    for rows in RAGGED:
        for cols in RAGGED:
            cs.append(SimpleNamespace(rows=rows, cols=cols, lds=cols + 5, ldd=rows + 7))
    for i, c in enumerate(cs):
        c.name = "t%dx%d" % (c.rows, c.cols)
        c.src = shadow_data(c.rows * c.lds, 500 + i)
    return cs
