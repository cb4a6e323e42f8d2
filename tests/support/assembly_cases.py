"""TEST INFRASTRUCTURE -- the direct-mode cases of the assembly kernel's edge tests (tests/test_gpu_assembly_edges.py,
tests/test_assembly_reference_cpu.py): shapes at every layout decision of ``k_assemble``, seeded inputs.

A workgroup of 256 threads handles cw = min(q, 256) columns side by side on rpp = 256 // cw row lanes; the shapes put
R below, at and above rpp and 256, q at every change of rpp and of the number of column passes (q > 256), and the
scale-factor groups in every arrangement the per-lane partial sums and their flush have to survive.
Inputs: sims uniform(0.5, 3), data uniform(1, 2), sigma uniform(0.05, 0.2), Jm standard normal -- every group's
sum s^2 / sigma^2 stays away from zero and every logarithm's argument positive."""
from __future__ import annotations

import numpy as np

SQUARE, LOG = 0, 1
V = 3


def row_lanes(q):
    return 256 // min(max(q, 1), 256)


def group_pattern(name, R, G, rpp, rng):
    """row -> scale-factor group (or -1) for the named arrangement"""
    if G == 0:
        return np.full(R, -1, dtype=np.int32)
    r = np.arange(R)
    if name == 'contiguous':
        g = r * G // R
    elif name == 'interleaved':
        g = r % G
    elif name == 'interleaved_gaps':          # 0, -1, 1, -1, 2, -1, ...
        g = np.where(r % 2 == 0, (r // 2) % G, -1)
    elif name == 'single_row':                # group 0 is one row in the middle, the others interleaved
        g = 1 + r % (G - 1)
        g[R // 2] = 0
    elif name == 'one_lane':                  # group 0 = the rows of ONE row lane (r = c mod rpp), the rest random
        assert rpp > 1 and R > rpp
        g = rng.integers(1, G, R) if G > 1 else np.full(R, -1)
        others = np.flatnonzero(r % rpp != 0)
        g[others[1:G]] = np.arange(1, G)
        g[r % rpp == 0] = 0
    elif name == 'first_last':                # group 0 = first and last row, the other groups contiguous between
        g = 1 + (r - 1) * (G - 1) // max(R - 2, 1) if G > 1 else np.full(R, -1)
        g[0] = g[R - 1] = 0
    elif name == 'random':
        g = rng.integers(-1, G, R)
        g[rng.permutation(R)[:G]] = np.arange(G)
    else:
        raise ValueError(name)
    return np.asarray(g, dtype=np.int32)


# (q, R, G, pattern, loss, reference_compat, sf priors, plain rows, non-positive simulation in vector 2)
_SHAPES = [
    (1, 1, 0, 'contiguous', SQUARE, 0, False, False, False),
    (1, 2, 1, 'contiguous', LOG, 1, False, False, False),
    (1, 255, 3, 'interleaved', SQUARE, 1, True, False, False),
    (1, 256, 7, 'random', LOG, 0, True, False, False),
    (1, 257, 3, 'interleaved_gaps', SQUARE, 0, False, False, False),
    (2, 127, 3, 'single_row', SQUARE, 0, True, False, False),
    (2, 128, 1, 'contiguous', LOG, 0, False, True, False),
    (2, 129, 7, 'one_lane', SQUARE, 1, False, False, False),
    (3, 84, 3, 'first_last', LOG, 1, True, False, False),
    (3, 85, 7, 'interleaved', SQUARE, 0, False, False, False),
    (3, 86, 3, 'one_lane', LOG, 0, True, True, False),
    (3, 86, 3, 'one_lane', LOG, 0, True, True, True),
    (63, 3, 1, 'contiguous', SQUARE, 0, False, False, False),
    (63, 700, 7, 'random', SQUARE, 0, True, False, False),
    (64, 4, 3, 'interleaved', LOG, 0, False, False, False),
    (64, 5, 0, 'contiguous', SQUARE, 1, False, False, False),
    (65, 2, 1, 'contiguous', SQUARE, 0, False, False, False),
    (65, 257, 3, 'interleaved_gaps', LOG, 1, False, True, False),
    (85, 3, 3, 'interleaved', SQUARE, 0, True, False, False),
    (85, 256, 7, 'first_last', SQUARE, 1, False, False, False),
    (86, 1, 1, 'contiguous', LOG, 0, True, False, False),
    (86, 255, 3, 'one_lane', SQUARE, 0, False, False, False),
    (127, 3, 1, 'first_last', SQUARE, 0, False, False, False),
    (128, 2, 1, 'contiguous', LOG, 1, False, False, False),
    (128, 700, 7, 'interleaved_gaps', SQUARE, 0, True, False, False),
    (129, 1, 0, 'contiguous', SQUARE, 0, False, False, False),
    (129, 256, 3, 'random', LOG, 0, False, False, False),
    (255, 2, 1, 'contiguous', SQUARE, 1, False, False, False),
    (256, 257, 3, 'interleaved', LOG, 1, True, False, False),
    (257, 255, 7, 'interleaved_gaps', SQUARE, 0, True, False, False),
    (300, 2, 1, 'contiguous', LOG, 0, False, True, False),
    (300, 256, 3, 'single_row', SQUARE, 0, False, False, False),
    (513, 1, 1, 'contiguous', LOG, 1, False, False, False),
    (513, 257, 3, 'first_last', SQUARE, 0, True, False, False),
]


def case_id(shape):
    q, R, G, pat, loss, compat, pri, plain, nonpos = shape
    return "q%d-R%d-G%d-%s-%s-compat%d%s%s%s" % (q, R, G, pat, 'log' if loss else 'square', compat, '-sfprior' if pri else '',
                                                 '-plain' if plain else '', '-nonpositive' if nonpos else '')


SHAPES = _SHAPES
IDS = [case_id(s) for s in SHAPES]


class Case(object):
    """The arrays of one case; built from its shape and a seed that depends on nothing else."""

    def __init__(self, shape):
        q, R, G, pat, loss, compat, pri, plain, nonpos = shape
        self.shape, self.id = shape, case_id(shape)
        self.q, self.R, self.G, self.loss, self.compat, self.nonpositive = q, R, G, loss, compat, nonpos
        rng = np.random.default_rng([q, R, G, loss, compat, int(pri), int(plain)])
        self.rpp = row_lanes(q)
        self.group = group_pattern(pat, R, G, self.rpp, rng)
        self.plain = None
        if plain:
            assert loss == LOG
            # plain rows carry no group: every fifth row leaves its group, and the ungrouped rows alternate plain / log
            self.group[np.arange(R) % 5 == 1] = -1
            free = np.flatnonzero(self.group < 0)
            self.plain = np.zeros(R, dtype=np.int32)
            self.plain[free[::2]] = 1
            assert self.plain.any()
        self.data = rng.uniform(1.0, 2.0, R)
        self.sigma = rng.uniform(0.05, 0.2, R)
        self.sims = rng.uniform(0.5, 3.0, (V, R))
        self.Jm = rng.standard_normal((V, R, q))
        groups = np.arange(0, G, 2) if pri else np.zeros(0, dtype=int)
        self.sfp_group = groups.astype(np.int32)
        self.sfp_mean = rng.uniform(-0.5, 0.5, len(groups))
        self.sfp_sigma = rng.uniform(0.3, 1.0, len(groups))
        self.nan_row = int(rng.integers(0, R))                  # vector 1's NaN
        logrows = np.flatnonzero(self.plain == 0) if self.plain is not None else np.arange(R)
        self.nonpos_row = int(logrows[len(logrows) // 2])       # vector 2's non-positive simulation (log loss)
        self.counts = np.bincount(self.group[self.group >= 0], minlength=G)

    def sf_prior(self):
        return (self.sfp_group, self.sfp_mean, self.sfp_sigma) if len(self.sfp_group) else None

    def sims_with_faults(self):
        s = self.sims.copy()
        s[1, self.nan_row] = np.nan
        if self.nonpositive:
            s[2, self.nonpos_row] = -0.25 if self.nonpos_row % 2 else 0.0
        return s
