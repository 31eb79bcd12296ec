"""Drop-in for the reference's Cython module ``ctc_fast/swbd-utils/editDist.pyx`` (used by
errorAnalysis.py, compare_errs.py and edAlign.py): the table and the operation path come from
the MI355X (:func:`ctc_fast.edit_distance_batch`, a = hyp, b = ref), the aligned pair and
``errs_by_pos`` are read off the path on the host.

    edit_distance(hyp, ref) -> (ed, eq, ins, dels, subs, errs_by_pos, hyp_corr, ref_corr)   editDist.pyx:34-108
    ref_to_hyp(hyp_corr, ref_corr) -> r2h                                                   editDist.pyx:12-31

Here ``dels`` counts hypothesis tokens without a partner (``'<del>'`` in ref_corr) and ``ins``
reference tokens without one (``'<ins>'`` in hyp_corr), as the reference names them.
:func:`edit_distance_many` scores a list of pairs in one launch.  There is no CPU fallback.
"""
import numpy as np

import ctc_fast
from editDistance import _ids


def ref_to_hyp(hyp_corr, ref_corr):
    """For every reference token of an aligned pair, the index of its hypothesis token; a reference token
    without a partner (``'<ins>'`` above it) gets the index of the next hypothesis token (editDist.pyx:12-31)."""
    r2h, seen = [], 0                       # seen: hypothesis tokens to the left of this column
    for h, r in zip(hyp_corr, ref_corr):
        if r != '<del>':
            r2h.append(seen)
        if h != '<ins>':
            seen += 1
    return r2h


def _derive(hyp, ref, stats, path):
    """the return tuple of editDist.pyx:108 from the five counts and the forward path"""
    m = len(hyp)
    ed, dels, ins, subs, eq = (int(v) for v in stats)
    errs_by_pos = np.zeros(m, dtype=np.int64)
    hyp_corr, ref_corr = [], []
    # The trace-back stops where the first sequence runs out (editDist.pyx:69); what is left of the other (j
    # hypothesis tokens or k reference tokens, never both) is the head of the path and is booked in one
    # lump at errs_by_pos[max(j-1, 0)] (editDist.pyx:96-97), not token by token.
    head = 0
    while head < len(path) and path[head] == path[0] and path[0] in (ctc_fast.OP_UP, ctc_fast.OP_LEFT):
        head += 1
    j = k = 0            # tokens of hyp / ref consumed so far
    if head and m > 0:
        errs_by_pos[max(head - 1, 0) if path[0] == ctc_fast.OP_UP else 0] += head
    for pos, op in enumerate(path):
        if op == ctc_fast.OP_UP:                  # a hypothesis token alone
            hyp_corr.append(hyp[j])
            ref_corr.append('<del>')
            if pos >= head:
                errs_by_pos[j] += 1
            j += 1
        elif op == ctc_fast.OP_LEFT:              # a reference token alone
            hyp_corr.append('<ins>')
            ref_corr.append(ref[k])
            if pos >= head:
                errs_by_pos[j - 1] += 1           # editDist.pyx:83: the hypothesis position it follows
            k += 1
        else:
            hyp_corr.append(hyp[j])
            ref_corr.append(ref[k])
            if op == ctc_fast.OP_SUB:
                errs_by_pos[j] += 1
            j += 1
            k += 1
    return ed, eq, ins, dels, subs, errs_by_pos, hyp_corr, ref_corr


def edit_distance_many(hyps, refs):
    """the tuples of :func:`edit_distance` for the pairs (hyps[i], refs[i]), one launch"""
    hyps, refs = [list(h) for h in hyps], [list(r) for r in refs]
    if len(refs) != len(hyps):
        raise ValueError("edit_distance_many: %d hypotheses for %d references" % (len(hyps), len(refs)))
    ids = _ids(hyps + refs)
    stats, paths = ctc_fast.edit_distance_batch(ids[:len(hyps)], ids[len(hyps):], ops=True)
    return [_derive(h, r, s, p) for h, r, s, p in zip(hyps, refs, stats, paths)]


def edit_distance(hyp, ref):
    """(ed, eq, ins, dels, subs, errs_by_pos, hyp_corr, ref_corr) of one pair: the distance, its split into
    equal, inserted, deleted and substituted tokens, the errors booked per hypothesis position, and the two
    sequences aligned column by column with ``'<ins>'`` / ``'<del>'`` in the gaps"""
    return edit_distance_many([hyp], [ref])[0]
