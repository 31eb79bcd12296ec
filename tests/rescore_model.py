"""Float64 restatement of the combine-and-rank step of n-best rescoring (nbest_rank_kernel in csrc/lm_score.hip,
DESIGN.md §4.12), in plain Python floats: the yardstick of tests/test_gpu_rescore.py.

    real(b, k)      k < K_b[b], and -- where the first pass's scores are given -- no rank 0..k of utterance b is at
                    -inf there (the searches fill the ranks beyond the beam with "empty, -inf")
    rescored[b, k]  (total + alpha * lm) + beta * U for a real hypothesis with align status 0, the operation order of
                    ctc_fast.score_sentences; otherwise -inf
    order[b]        the real ranks by descending rescored value, ties to the lower first-pass rank; then the ranks
                    that are not real, in their original order

``tie`` and ``assoc`` exist for the mutation checks of tests/test_rescore_model_cpu.py only."""
import numpy as np

NEG = float("-inf")


def combine(total, lm, U, alpha, beta, assoc="left"):
    total, lm, alpha, beta = float(total), float(lm), float(alpha), float(beta)
    if assoc == "left":
        return (total + alpha * lm) + beta * float(U)
    return total + (alpha * lm + beta * float(U))          # the mutation: reassociated


def real_count(K_b, first):
    kb = int(K_b)
    if first is not None:
        for k in range(kb):
            if first[k] == NEG:
                return k
    return kb


def rank(total, status, lm, U, K_b, alpha, beta, first=None, tie="low", assoc="left"):
    """total, status, U [B, K]; lm [B, K] or None; K_b [B]; first [B, K] or None -> (order int32 [B, K],
    rescored float64 [B, K])"""
    total = np.asarray(total, dtype=np.float64)
    B, K = total.shape
    rescored = np.full((B, K), NEG, dtype=np.float64)
    order = np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        kb = real_count(K_b[b], None if first is None else first[b])
        for k in range(kb):
            if status[b][k] == 0:
                rescored[b, k] = combine(total[b, k], 0.0 if lm is None else lm[b][k], U[b][k], alpha, beta, assoc)
        sign = 1 if tie == "low" else -1                     # the mutation: ties to the higher rank
        ranked = sorted(range(kb), key=lambda k: (-rescored[b, k], sign * k))
        order[b] = ranked + list(range(kb, K))
    return order, rescored
