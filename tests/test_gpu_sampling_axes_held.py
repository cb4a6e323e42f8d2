"""``sbm_sampling_axes_held`` against ``sbm_sampling_axes`` on the reduced arrays (the held columns deleted), one reduced
call per chain: the free part bit for bit, the padding exact zeros and ones (include/sbm.h)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T_AXES, STEP_AXES, CUTOFF = 1.5, 0.7, 1e-4


def _call(C, q, J=None, row_scale=None, H=None, per_chain=0, held=None, entry='held', cutoff=CUTOFF):
    """(rc, eig, V, s, samp, status); the outputs start as 7 so that an entry the kernel leaves alone shows"""
    import torch
    from sysbio_modeling_amd import _lib
    ctx = _lib.default_context()
    p = _lib.dev_ptr
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    Jd, rd, Hd = up(J), up(row_scale), up(H)
    hd = None if held is None else torch.from_numpy(np.ascontiguousarray(held, dtype=np.int32)).cuda()
    M = 0 if J is None else J.shape[1]
    eig, s = (torch.full((C, q), 7.0, dtype=torch.float64, device='cuda') for _ in range(2))
    V, samp = (torch.full((C, q, q), 7.0, dtype=torch.float64, device='cuda') for _ in range(2))
    status = torch.full((C,), 7, dtype=torch.int32, device='cuda')
    args = (ctx.handle, p(Jd), p(rd), p(Hd), per_chain, C, M, q, float(cutoff), T_AXES, STEP_AXES, p(eig), p(V), p(s), p(samp),
            p(status))
    rc = ctx.lib.sbm_sampling_axes_held(*args, p(hd)) if entry == 'held' else ctx.lib.sbm_sampling_axes(*args)
    torch.cuda.synchronize()
    return (rc,) + tuple(x.cpu().numpy() for x in (eig, V, s, samp, status))


def _expected(q, masks, reduced):
    """The padded layout from the reduced outputs: ``reduced(c, free)`` -> (eig, V, s, samp) of chain c's reduced problem"""
    C = len(masks)
    eig, s = np.zeros((C, q)), np.ones((C, q))
    V, samp = np.zeros((C, q, q)), np.zeros((C, q, q))
    for c, mask in enumerate(masks):
        free = np.flatnonzero(~mask)
        nf = free.size
        if nf == 0:
            continue
        e, v, sr, m = reduced(c, free)
        eig[c, :nf], s[c, :nf] = e, sr
        V[c][np.ix_(free, np.arange(nf))] = v
        samp[c][np.ix_(free, np.arange(nf))] = m
    return eig, V, s, samp


def _masks_with_nf(q, nfs, rng):
    out = []
    for nf in nfs:
        m = np.ones(q, dtype=bool)
        m[rng.choice(q, nf, replace=False)] = False
        out.append(m)
    return out


def _shape_masks(shape):
    C, M, q = shape
    rng = np.random.default_rng(q)
    if q == 7:
        eye = np.eye(q, dtype=bool)
        return [np.zeros(q, bool), eye[0], eye[q - 1], ~eye[4], np.ones(q, bool), np.array([0, 1, 1, 0, 0, 1, 0], bool)]
    return _masks_with_nf(q, {33: (33, 32, 31, 2), 96: (95, 64)}[q], rng)


def _jacobians(C, M, q):
    rng = np.random.default_rng(1000 * q + M)
    return rng.standard_normal((C, M, q)) * 10.0 ** rng.uniform(-2.0, 2.0, q), rng.uniform(0.5, 20.0, M)


SHAPES = [(6, 20, 7), (4, 33, 33), (2, 40, 96)]


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda sh: 'C%d-M%d-q%d' % sh)
def test_held_axes_from_jacobians_are_the_reduced_problem(shape, scaled):
    """All masks of a shape in ONE launch: q = 7 with none held, the first, the last, all but one (nf = 1), all (nf = 0) and a
    mixed mask; q = 33 with nf = 33, 32, 31 and 2 (odd and even numbers of players of the round robin, the 32-row tile, a
    last tile of one row at M = 33); q = 96 with nf = 95 and 64 (the LDS maximum)."""
    C, M, q = shape
    J, scale = _jacobians(C, M, q)
    rs = scale if scaled else None
    masks = _shape_masks(shape)
    assert len(masks) == C
    rc, eig, V, s, samp, status = _call(C, q, J=J, row_scale=rs, held=np.stack(masks))
    assert rc == 0 and np.all(status == 0)

    def reduced(c, free):
        out = _call(1, free.size, J=J[c:c + 1][:, :, free], row_scale=rs, entry='plain')
        assert out[0] == 0 and out[5][0] == 0
        return tuple(x[0] for x in out[1:5])
    for got, want in zip((eig, V, s, samp), _expected(q, masks, reduced)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize('per_chain', [0, 1])
def test_held_axes_from_matrices_are_the_reduced_problem(per_chain):
    C, M, q = SHAPES[0]
    J, _ = _jacobians(C, M, q)
    H = np.einsum('cmi,cmj->cij', J, J)
    H = H + 0.01 * np.triu(H, 1)                    # not symmetric: used as (H + H^T) / 2
    Hin = H if per_chain else H[0]
    masks = _shape_masks(SHAPES[0])
    rc, eig, V, s, samp, status = _call(C, q, H=Hin, per_chain=per_chain, held=np.stack(masks))
    assert rc == 0 and np.all(status == 0)

    def reduced(c, free):
        Hc = H[c] if per_chain else H[0]
        out = _call(1, free.size, H=Hc[np.ix_(free, free)], entry='plain')
        assert out[0] == 0 and out[5][0] == 0
        return tuple(x[0] for x in out[1:5])
    for got, want in zip((eig, V, s, samp), _expected(q, masks, reduced)):
        assert np.array_equal(got, want)


def test_held_axes_special_inputs():
    """A NaN in a held column of J (or a held row / column of H) is not looked at; one in a free column is status 1 for that
    chain only, with V = samp = 0 and s = eig = NaN on all q entries; held = NULL is sbm_sampling_axes."""
    C, M, q = SHAPES[0]
    J, scale = _jacobians(C, M, q)
    masks = np.stack(_shape_masks(SHAPES[0]))
    good = _call(C, q, J=J, held=masks)
    Jn = J.copy()
    for c in range(C):
        Jn[c, 3 + c, masks[c]] = np.nan              # every held column of every chain
    out = _call(C, q, J=Jn, held=masks)
    assert out[0] == 0 and np.all(out[5] == 0)
    for x, y in zip(out[1:5], good[1:5]):
        assert np.array_equal(x, y)
    Jb = Jn.copy()
    Jb[5, 19, 0] = np.inf                            # chain 5: column 0 is free
    assert not masks[5, 0]
    rc, eig, V, s, samp, status = _call(C, q, J=Jb, held=masks)
    assert rc == 0 and list(status) == [0, 0, 0, 0, 0, 1]
    assert np.all(V[5] == 0.0) and np.all(samp[5] == 0.0) and np.all(np.isnan(s[5])) and np.all(np.isnan(eig[5]))
    for x, y in zip((eig, V, s, samp), good[1:5]):
        assert np.array_equal(x[:5], y[:5])
    H = np.einsum('cmi,cmj->cij', J, J)
    Hn = H.copy()
    for c in range(C):
        Hn[c, masks[c], :] = np.nan
        Hn[c, :, masks[c]] = np.inf
    a, b = _call(C, q, H=Hn, per_chain=1, held=masks), _call(C, q, H=H, per_chain=1, held=masks)
    assert a[0] == 0 and np.all(a[5] == 0)
    for x, y in zip(a[1:5], b[1:5]):
        assert np.array_equal(x, y)
    Hb = Hn.copy()
    Hb[2, 3, 1] = np.nan                             # chain 2 holds the last column only
    assert list(_call(C, q, H=Hb, per_chain=1, held=masks)[5]) == [0, 0, 1, 0, 0, 0]
    # no mask at all: the kernel of sbm_sampling_axes
    for kw in (dict(J=J, row_scale=scale), dict(H=H, per_chain=1)):
        for x, y in zip(_call(C, q, held=None, **kw), _call(C, q, entry='plain', **kw)):
            assert np.array_equal(x, y)
    # and the reduced recipe is the reduced problem's: nf = 1 has n_eff = 1 and s = step sqrt(T) / sqrt(a)
    only = int(np.flatnonzero(~masks[3])[0])
    a3 = 0.5 * np.sum(J[3][:, only] ** 2)
    assert np.isclose(good[1][3, 0], a3, rtol=1e-14) and np.isclose(good[3][3, 0], STEP_AXES * np.sqrt(T_AXES / a3), rtol=1e-14)
