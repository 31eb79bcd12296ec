"""Drop-in for the reference's ``ctc_fast/editDistance.py``: the same two functions, the
table and the trace-back (editDistance.py:14-45) computed on the MI355X by
:func:`ctc_fast.edit_distance_batch`.

    edit_distance(ref, hyp) -> (dist, ins, dels, subs, corr)      editDistance.py:3-45
    disp(ref, hyp)                                                editDistance.py:47-51

``ref`` and ``hyp`` are sequences of hashable tokens (characters, words, ids).  The naming is
the reference's: the counts "transform hyp to ref", so a reference token missing from the
hypothesis is an insertion.  :func:`edit_distance_many` scores a list of pairs in one launch.
There is no CPU fallback.
"""
import ctc_fast


def _ids(seqs):
    """tokens -> dense ids shared by all the sequences (equality is all the table looks at)"""
    table = {}
    return [[table.setdefault(t, len(table)) for t in s] for s in seqs]


def edit_distance_many(refs, hyps):
    """[(dist, ins, dels, subs, corr)] of the pairs (refs[i], hyps[i]), one launch"""
    refs, hyps = list(refs), list(hyps)
    if len(refs) != len(hyps):
        raise ValueError("edit_distance_many: %d references for %d hypotheses" % (len(refs), len(hyps)))
    ids = _ids(refs + hyps)
    stats = ctc_fast.edit_distance_batch(ids[:len(refs)], ids[len(refs):])
    # editDistance.py:45 returns D[-1,-1] of a float table
    return [(float(s[0]), int(s[1]), int(s[2]), int(s[3]), int(s[4])) for s in stats]


def edit_distance(ref, hyp):
    """(float(dist), ins, dels, subs, corr) of one pair: ``ins`` reference tokens the hypothesis lacks,
    ``dels`` hypothesis tokens the reference lacks, ``subs`` replaced and ``corr`` equal tokens"""
    return edit_distance_many([ref], [hyp])[0]


def disp(ref, hyp):
    """prints the pair and its statistics in the three lines of the reference's report"""
    stats = edit_distance(ref, hyp)
    report = ["Reference : %s, Hypothesis : %s" % ("".join(ref), "".join(hyp)),
              "Distance : %d" % stats[0],
              "Ins : %d, Dels : %d, Subs : %d, Corr : %d" % stats[1:]]
    print("\n".join(report))
