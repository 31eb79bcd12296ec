"""A restatement of the edit-distance contract (include/sctc.h) for the tests:
the table of ctc_fast/editDistance.py:14-24, the trace-back rule of :29-43 (MATCH before UP
before LEFT before SUB, the leftovers as UP / LEFT), the path in forward order, and the counts
carried forward through the table, which is how the kernel gets them without a trace-back.

Also a restatement, in those terms, of what swbd-utils/editDist.pyx:40-108 returns, for the outputs
that stanford-ctc_amd/editDist.py derives from the path.  editDist.pyx itself cannot be run as a
reference here: the installed Cython rejects its ``np.int_t`` declarations (the alias left
NumPy), so tests/golden/edit_ref.npz records the outputs of editDistance.py only and the
restatement below is checked against hand-worked cases (tests/test_edit_distance_cpu.py).
"""
import numpy as np

MATCH, UP, LEFT, SUB = 0, 1, 2, 3


def table(a, b):
    """D and the operation of every cell (row 0 and column 0: LEFT and UP), vectorised over anti-diagonals"""
    a = np.asarray(a, dtype=np.int64).reshape(-1)
    b = np.asarray(b, dtype=np.int64).reshape(-1)
    n, m = a.shape[0], b.shape[0]
    D = np.zeros((n + 1, m + 1), dtype=np.int32)
    D[:, 0] = np.arange(n + 1)
    D[0, :] = np.arange(m + 1)
    op = np.zeros((n + 1, m + 1), dtype=np.int8)
    op[1:, 0] = UP
    op[0, 1:] = LEFT
    for k in range(2, n + m + 1):
        i = np.arange(max(1, k - m), min(n, k - 1) + 1)
        j = k - i
        up, left, diag = D[i - 1, j], D[i, j - 1], D[i - 1, j - 1]
        eq = a[i - 1] == b[j - 1]
        d = np.where(eq, diag, 1 + np.minimum(np.minimum(up, left), diag))
        D[i, j] = d
        op[i, j] = np.where(eq, MATCH, np.where(up == d - 1, UP, np.where(left == d - 1, LEFT, SUB)))
    return D, op


def trace(op, n, m):
    """(up, left, sub, match) and the forward path of the trace-back from (n, m)"""
    cnt = [0, 0, 0, 0]
    path = []
    i, j = n, m
    while i > 0 or j > 0:
        o = int(op[i, j])            # on the borders the stored operation is the leftover rule
        path.append(o)
        cnt[o] += 1
        i -= o != LEFT
        j -= o != UP
    return (cnt[UP], cnt[LEFT], cnt[SUB], cnt[MATCH]), np.array(path[::-1], dtype=np.int8)


def edit_model(a, b):
    """(stats int32[5] = dist, up, left, sub, match; path int8[]) of the contract"""
    D, op = table(a, b)
    n, m = D.shape[0] - 1, D.shape[1] - 1
    (u, l, s, e), path = trace(op, n, m)
    return np.array([D[n, m], u, l, s, e], dtype=np.int32), path


def edit_model_loop(a, b):
    """The same with plain loops, and the counts carried FORWARD through the table:
    cnt[i][j] = cnt[predecessor by the rule] + the operation, cnt[i][0] = i UPs, cnt[0][j] = j LEFTs.
    Returns (stats from the forward counts, stats from the trace-back, path)."""
    a, b = list(a), list(b)
    n, m = len(a), len(b)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    op = [[LEFT] * (m + 1) for _ in range(n + 1)]
    cnt = [[None] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        D[i][0], op[i][0], cnt[i][0] = i, UP, (i, 0, 0, 0)
    for j in range(m + 1):
        D[0][j], cnt[0][j] = j, (0, j, 0, 0)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            if a[i - 1] == b[j - 1]:
                D[i][j], o, prev = D[i - 1][j - 1], MATCH, cnt[i - 1][j - 1]
            else:
                D[i][j] = 1 + min(D[i - 1][j], D[i][j - 1], D[i - 1][j - 1])
                if D[i - 1][j] == D[i][j] - 1:
                    o, prev = UP, cnt[i - 1][j]
                elif D[i][j - 1] == D[i][j] - 1:
                    o, prev = LEFT, cnt[i][j - 1]
                else:
                    o, prev = SUB, cnt[i - 1][j - 1]
            op[i][j] = o
            c = list(prev)
            c[(UP, LEFT, SUB, MATCH).index(o)] += 1
            cnt[i][j] = tuple(c)
    (u, l, s, e), path = trace(np.array(op, dtype=np.int8).reshape(n + 1, m + 1), n, m)
    fwd = np.array((D[n][m],) + cnt[n][m], dtype=np.int32)
    return fwd, np.array([D[n][m], u, l, s, e], dtype=np.int32), path


def apply_path(a, b, path):
    """Walks `path` over a and b: MATCH copies a symbol of a (which must equal b's), UP drops one, LEFT
    takes b's, SUB replaces a's by b's (which must differ).  Returns the sequence built and the number of
    symbols of a consumed: a correct path builds b and consumes all of a."""
    a, b = list(a), list(b)
    i = j = 0
    out = []
    for o in path:
        if o == MATCH:
            assert a[i] == b[j]
            out.append(a[i])
        elif o == SUB:
            assert a[i] != b[j]
            out.append(b[j])
        elif o == LEFT:
            out.append(b[j])
        i += o != LEFT
        j += o != UP
    return out, i


def editdist_restated(hyp, ref):
    """The return tuple of swbd-utils/editDist.pyx (see the module docstring) in the terms of the contract
    with a = hyp, b = ref: UP is a hypothesis token alone (``dels``, ``'<del>'`` under it), LEFT a reference
    token alone (``ins``, ``'<ins>'`` above it).  What editDist.pyx does beyond the contract is the booking of
    errs_by_pos: an error of cell (j, k) goes to hypothesis position j - 1, and the leftovers of the border,
    j or k of them, go in one lump to position max(j - 1, 0) when the hypothesis is not empty."""
    hyp, ref = list(hyp), list(ref)
    ids = {}
    a, b = ([ids.setdefault(t, len(ids)) for t in s] for s in (hyp, ref))
    D, op = table(a, b)
    j, k = len(hyp), len(ref)
    cells = []                              # the interior cells of the path, from (m, n) back to the border
    while j > 0 and k > 0:
        o = int(op[j, k])
        cells.append((j, k, o))
        j -= o != LEFT
        k -= o != UP
    n_op = [sum(o == code for _, _, o in cells) for code in (MATCH, UP, LEFT, SUB)]
    errs_by_pos = np.zeros(len(hyp), dtype=np.int64)
    for jj, _, o in cells:
        errs_by_pos[jj - 1] += o != MATCH
    if hyp:
        errs_by_pos[max(j - 1, 0)] += j + k
    columns = [(t, '<del>') for t in hyp[:j]] + [('<ins>', t) for t in ref[:k]]      # one of the two is empty
    for jj, kk, o in reversed(cells):
        columns.append((hyp[jj - 1] if o != LEFT else '<ins>', ref[kk - 1] if o != UP else '<del>'))
    return (int(D[-1, -1]), n_op[MATCH], n_op[LEFT] + k, n_op[UP] + j, n_op[SUB], errs_by_pos,
            [h for h, _ in columns], [r for _, r in columns])


def random_pairs(seed, count, max_len, alphabets):
    """seeded pairs: lengths 0..max_len, alphabet sizes cycling through `alphabets`; half of the b are edits
    of their a, so that long matching runs and ties both occur"""
    rs = np.random.RandomState(seed)
    pairs = []
    for p in range(count):
        A = alphabets[p % len(alphabets)]
        n = int(rs.randint(0, max_len + 1))
        a = rs.randint(0, A, size=n).astype(np.int32)
        if p % 2:
            b = list(a)
            for _ in range(int(rs.randint(0, max(2, n // 3)))):
                kind, pos = rs.randint(3), int(rs.randint(0, len(b) + 1))
                if kind == 0:
                    b.insert(pos, int(rs.randint(0, A)))
                elif kind == 1 and b:
                    del b[min(pos, len(b) - 1)]
                elif b:
                    b[min(pos, len(b) - 1)] = int(rs.randint(0, A))
            b = np.array(b[:max_len], dtype=np.int32)
        else:
            b = rs.randint(0, A, size=int(rs.randint(0, max_len + 1))).astype(np.int32)
        pairs.append((a, b))
    return pairs
