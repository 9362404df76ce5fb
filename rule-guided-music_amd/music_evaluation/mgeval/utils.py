"""The three names of the reference's music_evaluation/mgeval/utils.py with its signatures, on float64 device tensors (csrc/sets.hip
through music_evaluation/set_eval.py).  Nothing is copied to the host; the results are 0-d or 1-d float64 device tensors.

Differences from the reference (docs/rounds/sets.md): c_dist serves mode='None' only (the evaluator uses no other) and writes NaN and
inf distances as 0, which music_evaluator.delete_nan does to them one step later; overlap_area is a composite Simpson rule on 16384
panels in place of QUADPACK's adaptive rule; where a variance is 0 kl_dist and overlap_area return NaN and the reference raises
LinAlgError."""
from .. import set_eval


def c_dist(A, B, mode='None', normalize=0):
    """Euclidean distance of the one sample A ((d,) or (1, d)) from every row of B (n, d) -> (n,)"""
    if mode != 'None':
        raise NotImplementedError(f"c_dist mode {mode!r}: only 'None' (Euclidean) is provided; music_evaluator.py uses no other")
    b = B.reshape(B.shape[0], -1)
    a = A.reshape(1, -1)
    return set_eval._distances(set_eval._f64(a), set_eval._f64(b), False)


def kl_dist(A, B, num_sample=1000):
    """scipy.stats.entropy of the Gaussian-KDE density of A on linspace(min A, max A, num_sample) against that of B on
    linspace(min B, max B, num_sample)"""
    return set_eval.kl_oa(A, B, kl_points=num_sample)[0]


def overlap_area(A, B):
    """the integral of min(pdf_A, pdf_B) over [min(min A, min B), max(max A, max B)]"""
    return set_eval.kl_oa(A, B)[1]
