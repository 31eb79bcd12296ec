"""What the GPU tests of the four prefix beam searches share below ``decode_beam_batch``: the C entry
points called on buffers the test lays out itself, and the comparison of two decoded batches."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHARS = os.path.join(ROOT, "tests", "golden", "chars.txt")
PATTERN = 0xA5


def int_char_map():
    """{symbol id: token} of tests/golden/chars.txt"""
    chars = {}
    with open(CHARS) as f:
        for l in f:
            t, i = l.split()
            chars[int(i)] = t
    return chars


def _config(search, handle, head, tail):
    """the config struct of an entry point: the lexicon search has its separator where the others have
    a reserved 0 and no symbol map; the character search may go without an LM"""
    import _sctc
    A = head[1]
    if search == "lexbeam":
        return _sctc.LexBeamConfig(*(head + (handle.space,) + tail + (handle.handle,)))
    cls = {"beam": _sctc.BeamConfig, "nnbeam": _sctc.NNBeamConfig, "rnnbeam": _sctc.RNNBeamConfig}[search]
    sw = np.ascontiguousarray(handle.sym_words[:A] if handle is not None else np.zeros(A, np.int32), dtype=np.int32)
    return cls(*(head + (0,) + tail + (handle.handle if handle is not None else None, _sctc.i32(sw))))


def raw_decode(search, host, ld, A, T_b, frame_off, beam, nbest, handle, alpha, beta, guard=0):
    """sctc_ctc_<search>_decode_batch (search: "beam", "lexbeam", "nnbeam" or "rnnbeam") on a host matrix
    [rows][ld] as it stands; handle: the ctc_fast.Decode* object of the search (None: "beam" without an
    LM).  With ``guard`` the workspace (exactly sctc_ctc_<search>_workspace_bytes, 256-byte aligned), ids,
    lengths and scores lie inside one pattern-filled buffer, ``guard`` bytes apart.  Returns (hyps,
    scores [B, nbest], lengths [B, nbest], the bytes outside the four, the workspace bytes)."""
    import torch
    import _sctc
    L = _sctc.lib()
    B = len(T_b)
    Tb = np.ascontiguousarray(T_b, dtype=np.int32)
    off = np.ascontiguousarray(frame_off, dtype=np.int64)
    dtype = _sctc.F64 if host.dtype == np.float64 else _sctc.F32
    cfg = _config(search, handle, (B, A, dtype, beam, nbest), (ld, _sctc.i32(Tb), _sctc.i64(off), alpha, beta))
    nbytes = getattr(L, "sctc_ctc_%s_workspace_bytes" % search)(ctypes.byref(cfg))
    assert nbytes > 0
    dev = torch.from_numpy(host).cuda()
    n_ids = max(1, nbest * int(Tb.sum()))
    sizes = [nbytes, 4 * n_ids, 4 * B * nbest, 8 * B * nbest]
    g = max(256, (guard + 255) // 256 * 256)
    offs, pos = [], g
    for s in sizes:
        offs.append(pos)
        pos = (pos + s + g + 255) // 256 * 256
    buf = torch.full((pos,), PATTERN, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    assert base % 256 == 0
    ws, ids, lens, scores = (base + o for o in offs)
    rc = getattr(L, "sctc_ctc_%s_decode_batch" % search)(ctypes.byref(cfg), dev.data_ptr(), ids, lens, scores, ws,
                                                         nbytes, _sctc.current_stream_ptr())
    _sctc.check(rc, "raw_decode")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    inside = np.zeros(pos, dtype=bool)
    for o, s in zip(offs, sizes):
        inside[o:o + s] = True
    ids_h = out[offs[1]:offs[1] + sizes[1]].view(np.int32)
    lens_h = out[offs[2]:offs[2] + sizes[2]].view(np.int32).copy()
    scores_h = out[offs[3]:offs[3] + sizes[3]].view(np.float64).reshape(B, nbest).copy()
    hyps, b0 = [], 0
    for b in range(B):
        hyps.append([ids_h[b0 + n * Tb[b]:b0 + n * Tb[b] + lens_h[b * nbest + n]].copy() for n in range(nbest)])
        b0 += nbest * int(Tb[b])
    return hyps, scores_h, lens_h.reshape(B, nbest), out[~inside], nbytes


def same_results(h1, s1, h2, s2, nbest):
    """scores and hypotheses array-equal; either side may list its hypotheses per utterance (raw_decode
    always, decode_beam_batch with nbest > 1) or give the one hypothesis itself (nbest == 1)"""
    np.testing.assert_array_equal(np.asarray(s1).reshape(-1), np.asarray(s2).reshape(-1))
    assert len(h1) == len(h2)
    for a, b in zip(h1, h2):
        a = a if isinstance(a, list) else [a]
        b = b if isinstance(b, list) else [b]
        assert len(a) == len(b) == nbest
        for x, y in zip(a, b):
            assert np.asarray(x).ndim == 1 and np.asarray(y).ndim == 1
            np.testing.assert_array_equal(x, y)
