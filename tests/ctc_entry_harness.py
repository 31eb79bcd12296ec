"""A raw caller of sctc_ctc_workspace_bytes / sctc_ctc_loss_batch for tests/test_gpu_ctc_entry.py (no tests here),
in the style of tests/beam_harness.py: the test lays out every buffer itself.

`call` takes a batch -- a list of (y (A, T_b) float32 or float64, seq) -- and a layout:

  ld            row stride of probs / grad, >= A; the padding columns of probs hold NaN
  place, gaps   contiguous mode: utterances lie in memory in the order `place`, gaps[i] NaN rows in front of the i-th
                (frame_off follows: any order, with gaps)
  rowbase       True: the packed time-major minibatch of the BRNN engine -- utterances ranked longest first (ties by
                index), rowbase[t] = sum over t' < t of #{b : T_b > t'} (tests/test_gpu_brnn._packed_rowbase),
                frame_off[b] = rank of b, frame t of utterance b in row rowbase[t] + rank
  order         the order in which the utterances are passed to the entry (default: as given; the engine passes them in
                rank order, include/sctc.h promises only frame_off[b] = rank of b)
  label_junk    junk label ids laid between and around the label rows, which lie in the label array in reverse order
  workspace_fill  a byte value, or "leftover": the entry is first called on `leftover` (another batch, of the same
                workspace size or larger) in the same buffer

probs, grad, cost, skip, rowbase and the workspace each lie in a device buffer of their own, GUARD bytes of PATTERN on
either side; the workspace is exactly sctc_ctc_workspace_bytes long (minus ws_short) and 256-byte aligned; gap rows and
padding columns of grad hold PATTERN too.  One more row behind the utterances' rows holds NaN, and the guards of rowbase
hold ITS index: a kernel that read rowbase out of bounds would compute NaN and write that row, which the comparisons
see, and would not leave the buffers.  Results come back in the order the batch was given, with the raw buffers, and
`untouched` lists what changed outside the owned regions (columns < A of an utterance's own rows of grad, cost[0..B),
skip[0..B)).
"""
import ctypes

import numpy as np

PATTERN = 0xA5
GUARD = 4096


def packed_rowbase(Ts):
    Ts = np.asarray(Ts)
    alive = np.array([(Ts > t).sum() for t in range(Ts.max())])
    return np.concatenate([[0], np.cumsum(alive)[:-1]])


class _Region(object):
    """`nbytes` of a device buffer between two guards of PATTERN (guard_word: of that int32 word instead)"""

    def __init__(self, torch, nbytes, fill=PATTERN, guard_word=None):
        self.nbytes = int(nbytes)
        self.guard_word = guard_word
        self.buf = torch.full((2 * GUARD + (self.nbytes + 255) // 256 * 256,), PATTERN, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + GUARD
        if guard_word is not None:
            assert self.nbytes % 4 == 0
            self.buf.view(torch.int32)[:] = guard_word
        elif fill != PATTERN and self.nbytes:
            self.buf[GUARD:GUARD + self.nbytes] = fill

    def upload(self, torch, host):
        raw = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        assert raw.size == self.nbytes
        self.buf[GUARD:GUARD + self.nbytes] = torch.from_numpy(raw).cuda()

    def inside(self):
        return self.buf[GUARD:GUARD + self.nbytes].cpu().numpy()

    def guards_intact(self, torch):
        head, tail = self.buf[:GUARD], self.buf[GUARD + self.nbytes:]
        if self.guard_word is not None:
            head, tail, want = head.view(torch.int32), tail.view(torch.int32), self.guard_word
        else:
            want = PATTERN
        return bool((head == want).all().item()) and bool((tail == want).all().item())


def _batch_struct(_sctc, B, A, blank, dtype, ld, T_b, U_b, frame_off, labels, label_off, rowbase_ptr):
    return _sctc.CtcBatch(B, int(A), int(blank), dtype, int(ld), _sctc.i32(T_b), _sctc.i32(U_b), _sctc.i64(frame_off),
                          _sctc.i32(labels), _sctc.i64(label_off), ctypes.c_void_p(rowbase_ptr))


def workspace_bytes(batch, blank=0):
    """sctc_ctc_workspace_bytes of the batch under the switches in force"""
    import _sctc
    B = len(batch)
    A = batch[0][0].shape[0]
    T_b = np.array([y.shape[1] for y, _ in batch], dtype=np.int32)
    U_b = np.array([len(s) for _, s in batch], dtype=np.int32)
    zero = np.zeros(B, dtype=np.int64)
    lab = np.zeros(max(1, int(U_b.sum())), dtype=np.int32)
    dtype = _sctc.F64 if batch[0][0].dtype == np.float64 else _sctc.F32
    bt = _batch_struct(_sctc, B, A, blank, dtype, A, T_b, U_b, zero, lab, zero, None)
    return int(_sctc.lib().sctc_ctc_workspace_bytes(ctypes.byref(bt)))


def call(batch, blank=0, ld=None, place=None, gaps=None, rowbase=False, order=None, label_junk=None,
         workspace_fill=PATTERN, leftover=None, ws_short=0):
    import torch
    import _sctc
    L = _sctc.lib()
    B = len(batch)
    A = batch[0][0].shape[0]
    dt = batch[0][0].dtype
    assert dt in (np.float32, np.float64) and all(y.dtype == dt and y.shape[0] == A for y, _ in batch)
    ld = A if ld is None else int(ld)
    assert ld >= A
    Ts = [y.shape[1] for y, _ in batch]
    order = list(range(B)) if order is None else list(order)
    assert sorted(order) == list(range(B))

    # ---- the rows: rows_of[u] = the row of every frame of utterance u (as given), off[u] = its frame_off
    if rowbase:
        assert place is None and gaps is None
        ranked = sorted(range(B), key=lambda u: (-Ts[u], u))
        rank = {u: r for r, u in enumerate(ranked)}
        rb = packed_rowbase(Ts).astype(np.int64)
        rows_of = [rb[:Ts[u]] + rank[u] for u in range(B)]
        off = [rank[u] for u in range(B)]
        n_rows = int(sum(Ts))
    else:
        place = list(range(B)) if place is None else list(place)
        gaps = [0] * B if gaps is None else list(gaps)
        assert sorted(place) == list(range(B)) and len(gaps) == B
        rows_of, off, at = [None] * B, [0] * B, 0
        for u, gap in zip(place, gaps):
            at += gap
            off[u] = at
            rows_of[u] = at + np.arange(Ts[u], dtype=np.int64)
            at += Ts[u]
        n_rows = at
    poison_row = n_rows                 # one NaN row more: where an out-of-bounds rowbase entry would lead
    probs_h = np.full((n_rows + 1, ld), np.nan, dtype=dt)
    owned = np.zeros((n_rows + 1, ld), dtype=bool)
    for u, (y, _) in enumerate(batch):
        probs_h[rows_of[u], :A] = y.T
        owned[rows_of[u], :A] = True
    assert owned[:, :A].sum() == A * sum(Ts)                                   # no row belongs to two utterances

    # ---- the labels: rows in reverse order of the batch, junk between and around them
    junk = [] if label_junk is None else [int(v) for v in label_junk]
    lab_parts, lab_off, at = [np.array(junk, dtype=np.int32)], [0] * B, len(junk)
    for u in reversed(range(B)):
        seq = np.asarray(batch[u][1], dtype=np.int32)
        lab_off[u] = at
        lab_parts += [seq, np.array(junk, dtype=np.int32)]
        at += len(seq) + len(junk)
    labels = np.ascontiguousarray(np.concatenate(lab_parts), dtype=np.int32)

    # ---- the descriptor, in the order the utterances are passed
    T_b = np.array([Ts[u] for u in order], dtype=np.int32)
    U_b = np.array([len(batch[u][1]) for u in order], dtype=np.int32)
    frame_off = np.array([off[u] for u in order], dtype=np.int64)
    label_off = np.array([lab_off[u] for u in order], dtype=np.int64)
    dtype = _sctc.F64 if dt == np.float64 else _sctc.F32

    r_rowbase = None
    if rowbase:
        r_rowbase = _Region(torch, 4 * max(Ts), guard_word=poison_row)
        r_rowbase.upload(torch, rb.astype(np.int32))
    bt = _batch_struct(_sctc, B, A, blank, dtype, ld, T_b, U_b, frame_off, labels, label_off,
                       r_rowbase.ptr if rowbase else None)
    nbytes = int(L.sctc_ctc_workspace_bytes(ctypes.byref(bt)))
    assert nbytes > 0, L.sctc_last_error()

    r_probs = _Region(torch, probs_h.nbytes)
    r_probs.upload(torch, probs_h)
    r_grad = _Region(torch, probs_h.nbytes)
    r_cost = _Region(torch, 8 * B)
    r_skip = _Region(torch, 4 * B)
    r_ws = _Region(torch, nbytes, fill=PATTERN if workspace_fill == "leftover" else int(workspace_fill))
    stream = _sctc.current_stream_ptr()
    if workspace_fill == "leftover":
        # another batch through the same workspace first (packed, into buffers of its own)
        lA = leftover[0][0].shape[0]
        lT = np.array([y.shape[1] for y, _ in leftover], dtype=np.int32)
        lU = np.array([len(s) for _, s in leftover], dtype=np.int32)
        lfo = np.concatenate([[0], np.cumsum(lT)[:-1]]).astype(np.int64)
        llo = np.concatenate([[0], np.cumsum(lU)[:-1]]).astype(np.int64)
        llab = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.int32) for _, s in leftover]))
        lbt = _batch_struct(_sctc, len(leftover), lA, blank if blank < lA else 0, dtype, lA, lT, lU, lfo, llab, llo, None)
        lbytes = int(L.sctc_ctc_workspace_bytes(ctypes.byref(lbt)))
        assert nbytes <= lbytes, "the leftover batch must need at least the workspace of the batch under test"
        big = _Region(torch, lbytes)
        lp = torch.from_numpy(np.concatenate([np.ascontiguousarray(y.T) for y, _ in leftover], axis=0)).cuda()
        lg, lc, ls = torch.empty_like(lp), torch.empty(len(leftover), dtype=torch.float64, device="cuda"), \
            torch.empty(len(leftover), dtype=torch.int32, device="cuda")
        _sctc.check(L.sctc_ctc_loss_batch(ctypes.byref(lbt), lp.data_ptr(), lg.data_ptr(), lc.data_ptr(), ls.data_ptr(),
                                          big.ptr, lbytes, stream), "ctc_entry_harness: the leftover call")
        torch.cuda.synchronize()
        assert big.guards_intact(torch)
        r_ws = big          # the batch under test gets the front of that buffer, exactly nbytes of it
    rc = L.sctc_ctc_loss_batch(ctypes.byref(bt), r_probs.ptr, r_grad.ptr, r_cost.ptr, r_skip.ptr, r_ws.ptr,
                               nbytes - ws_short, stream)
    torch.cuda.synchronize()
    err = L.sctc_last_error() if rc else b""

    grad_raw = r_grad.inside().view(dt).reshape(n_rows + 1, ld)
    cost_raw, skip_raw, probs_raw = r_cost.inside(), r_skip.inside(), r_probs.inside()
    cost_h = cost_raw.view(np.float64).copy()
    skip_h = skip_raw.view(np.int32).copy()
    res = {"rc": rc, "error": err, "workspace_bytes": nbytes, "owned": owned, "grad_raw": grad_raw,
           "probs_raw": probs_raw.view(dt).reshape(n_rows + 1, ld), "probs_sent": probs_h, "cost_raw": cost_raw,
           "skip_raw": skip_raw}
    # (a leftover workspace is the front of a larger buffer: what lies behind its first nbytes the first call owned)
    regions = [("probs", r_probs), ("grad", r_grad), ("cost", r_cost), ("skip", r_skip), ("the workspace", r_ws)]
    if rowbase:
        regions.append(("rowbase", r_rowbase))
    changed = ["the guards of " + name for name, region in regions if not region.guards_intact(torch)]
    if rowbase and not (r_rowbase.inside().view(np.int32) == rb).all():
        changed.append("rowbase")
    if probs_raw.tobytes() != probs_h.tobytes():
        changed.append("probs")
    outside = ~np.repeat(owned, np.dtype(dt).itemsize, axis=1)
    if (grad_raw.view(np.uint8).reshape(n_rows + 1, -1)[outside] != PATTERN).any():
        changed.append("grad outside the owned columns and rows")
    if rc != 0:
        for name, raw in (("grad", grad_raw.view(np.uint8)), ("cost", cost_raw), ("skip", skip_raw)):
            if (raw != PATTERN).any():
                changed.append(name + " of a rejected call")
        if workspace_fill != "leftover" and (r_ws.inside() != int(workspace_fill)).any():
            changed.append("the workspace of a rejected call")
    res["untouched"] = changed
    # ---- results in the order the batch was given
    inv = {u: i for i, u in enumerate(order)}
    res["cost"] = np.array([cost_h[inv[u]] for u in range(B)])
    res["skip"] = np.array([bool(skip_h[inv[u]]) for u in range(B)])
    res["skip_words"] = np.array([skip_h[inv[u]] for u in range(B)])
    res["grads"] = [np.asfortranarray(grad_raw[rows_of[u], :A].T) for u in range(B)]
    return res
