"""Parallel tempering restated in numpy, for the tests of ``sbm_pt_swap`` and of ``ensemble_log_params_batch`` with a
temperature ladder: the swap rule on given arrays (`swap_step`), the whole loop with given random numbers (`replay`), and a
stand-in project with two basins (`DoubleWellProject`).  Nothing here imports the package's sampler.

Layout (the issue's, as include/sbm.h states it): C chains are C / K ladders of K contiguous rungs; chain c is rung c % K and
keeps its temperature; the n-th swap step has parity n % 2 and proposes the pairs of rungs (k, k + 1) with k % 2 == parity."""
import numpy as np


def lower_chains(C, K, parity):
    """indices of the lower chain of every pair a swap step of this parity proposes"""
    rung = np.arange(C) % K
    return np.flatnonzero((rung % 2 == parity) & (rung + 1 < K))


def swap_bound(T, F_curr, F_cross, i):
    """the right-hand side of the swap rule for the pairs (i, i + 1), evaluated in the order the kernel uses"""
    j = i + 1
    with np.errstate(over='ignore', invalid='ignore'):
        return (F_curr[i] - F_cross[j]) / T[i] + (F_curr[j] - F_cross[i]) / T[j]


def swap_step(K, parity, T, F_cross, log_u, curr, F_curr, n_swapped, slot=None, slot_F=None):
    """One swap step on copies of the arrays: (curr, F_curr, n_swapped, slot, slot_F, taken) with ``taken`` the lower chains
    of the exchanged pairs.  ``F_cross`` None: ``F_curr`` stands in.  A pair is exchanged iff both cross energies are finite
    and log_u[i] < bound (strict)."""
    C = len(F_curr)
    X = F_curr if F_cross is None else F_cross
    i = lower_chains(C, K, parity)
    with np.errstate(invalid='ignore'):
        take = np.isfinite(X[i]) & np.isfinite(X[i + 1]) & (log_u[i] < swap_bound(T, F_curr, X, i))
    i = i[take]
    j = i + 1
    curr, new_F, n_swapped = curr.copy(), F_curr.copy(), n_swapped.copy()
    curr[i], curr[j] = curr[j].copy(), curr[i].copy()
    new_F[i], new_F[j] = X[j], X[i]
    n_swapped[i] += 1
    if slot is not None:
        slot = slot.copy()
        slot[i], slot[j] = curr[i], curr[j]
    if slot_F is not None:
        slot_F = slot_F.copy()
        slot_F[i], slot_F[j] = new_F[i], new_F[j]
    return curr, new_F, n_swapped, slot, slot_F, i


def replay(energies, starts, samp, T, z, log_u, log_u_swap, swap_every=None, every=1, held=None, lower=None, upper=None):
    """The tempered loop with given draws.

    energies(theta (C, q)) -> (K, C): row k holds F(theta_c; T_k) for EVERY chain c (an energy that does not depend on the
    temperature repeats one row), +inf where a point cannot be evaluated.  ``samp`` (C, q, q) the chains' candidate
    matrices; ``held`` bool (C, q), ``lower`` / ``upper`` (C, q) or None.  Returns a dict: ens, ens_F, n_accepted,
    n_swapped, and the smallest |log u - bound| over all move decisions (``move_margin``) and all swap decisions
    (``swap_margin``) that an energy decided."""
    T = np.asarray(T, dtype=float)
    C, q = starts.shape
    K = len(T)
    rung, chains = np.arange(C) % K, np.arange(C)
    chain_T = T[rung]
    held = np.zeros((C, q), dtype=bool) if held is None else np.asarray(held, dtype=bool)
    lower = np.full((C, q), -np.inf) if lower is None else lower
    upper = np.full((C, q), np.inf) if upper is None else upper
    curr = starts.copy()
    Fc = energies(curr)[rung, chains]
    ens, ens_F = [curr.copy()], [Fc.copy()]
    n_acc, n_swapped = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64)
    move_margin = swap_margin = np.inf
    n_swaps = 0
    for n in range(len(z)):
        trial = np.where(held, curr, curr + np.einsum('cij,cj->ci', samp, z[n]))
        outside = (~((trial >= lower) & (trial <= upper)) & ~held).any(axis=1) | held.all(axis=1)
        trial = np.where(outside[:, None], curr, trial)
        Ft = energies(trial)[rung, chains]
        with np.errstate(invalid='ignore', over='ignore'):
            bound = -(Ft - Fc) / chain_T
            decided = np.isfinite(Ft) & ~outside
            acc = decided & (log_u[n] < bound)
            move_margin = min(move_margin, np.min(np.abs(log_u[n] - bound)[decided], initial=np.inf))
        curr, Fc = np.where(acc[:, None], trial, curr), np.where(acc, Ft, Fc)
        n_acc += acc
        if swap_every and (n + 1) % swap_every == 0:
            parity = n_swaps % 2
            i = lower_chains(C, K, parity)
            partner = chains.copy()
            partner[i], partner[i + 1] = i + 1, i
            X = energies(curr)[rung[partner], chains]
            ok = np.isfinite(X[i]) & np.isfinite(X[i + 1])
            swap_margin = min(swap_margin, np.min(np.abs(log_u_swap[n_swaps][i] - swap_bound(chain_T, Fc, X, i))[ok], initial=np.inf))
            curr, Fc, n_swapped, _, _, _ = swap_step(K, parity, chain_T, X, log_u_swap[n_swaps], curr, Fc, n_swapped)
            n_swaps += 1
        if (n + 1) % every == 0:
            ens.append(curr.copy())
            ens_F.append(Fc.copy())
    return dict(ens=np.stack(ens), ens_F=np.stack(ens_F), n_accepted=n_acc, n_swapped=n_swapped, move_margin=move_margin,
                swap_margin=swap_margin)


class DoubleWellProject:
    """Residuals r = ((theta_0^2 - 1) / width, theta_1): exp(-0.5 |r|^2) has two equal basins at theta_0 = +-1, separated by a
    barrier of 0.5 / width^2 at theta_0 = 0 (22 for width = 0.15), and a standard normal theta_1.  What the 'host' sampler
    asks of a project."""
    reference_compat = False
    scale_factors = None

    def __init__(self, width=0.15):
        self.width = float(width)

    def evaluate_batch(self, thetas, jacobian=False, want=(), **kw):
        th = np.atleast_2d(np.asarray(thetas, dtype=float))
        r = np.stack([(th[:, 0] ** 2 - 1.0) / self.width, th[:, 1]], axis=1)
        out = {'residuals': r, 'norms': np.sum(r * r, axis=1), 'status': np.zeros(len(r), dtype=np.int32)}
        if jacobian:
            J = np.zeros((len(th), 2, 2))
            J[:, 0, 0] = 2.0 * th[:, 0] / self.width
            J[:, 1, 1] = 1.0
            out['jacobian'] = J
        return out
