"""CPU: the float64 referee of the lazy-Adam row update (tests/adam_referee.py) is torch.optim.SparseAdam's own arithmetic, and
the error bound the GPU tests apply (adam_referee.tolerances) separates a correct fp32 implementation from one whose
hyper-parameters were rounded to fp32 first."""
import numpy as np
import pytest
import torch

import adam_referee as ar


def _step_inputs(g, N, U, d, M, n, with_pos=True):
    query = torch.randn(U, d, generator=g)
    qi = torch.randint(0, U, (M,), generator=g)
    neg = torch.randint(0, N, (M, n), generator=g)
    neg[torch.rand(M, n, generator=g) < 0.05] = -1
    pos = torch.randint(0, N, (M,), generator=g) if with_pos else None
    dneg = torch.randn(M, n, generator=g)
    dpos = torch.randn(M, generator=g) if with_pos else None
    return query, qi, neg, pos, dneg, dpos


@pytest.mark.parametrize('betas,pad_row', [((0.9, 0.999), 0), ((0.5, 0.9), -1)])
def test_referee_equals_torch_sparse_adam_in_float64(betas, pad_row):
    """Six steps with repeating rows (40 rows, ~330 elements a step; rows 30 .. 39 only from step 3 on, so that states of
    different ages coexist): weight, exp_avg, exp_avg_sq of the referee == torch.optim.SparseAdam on float64 parameters fed the COO
    gradient of the same elements, to 1e-12 absolute (inputs of order 1; measured 2e-16 / 5e-15 / 4e-15)."""
    g = torch.Generator().manual_seed(3)
    N, U, d, M, n, lr, eps = 40, 17, 8, 30, 10, 0.05, 1e-8
    w = torch.randn(N, d, generator=g)
    p = torch.nn.Parameter(w.double().clone())
    opt = torch.optim.SparseAdam([p], lr=lr, betas=betas, eps=eps)
    w, m, v = w.double(), torch.zeros(N, d, dtype=torch.float64), torch.zeros(N, d, dtype=torch.float64)
    up = torch.tensor([0.37])
    for step in range(1, 7):
        query, qi, neg, pos, dneg, dpos = _step_inputs(g, 30 if step < 3 else N, U, d, M, n)
        ref = ar.referee(w, m, v, query, neg, dneg, lr=lr, betas=betas, eps=eps, step=step, query_index=qi, pos_ids=pos, dpos=dpos,
                         upstream=up, pad_row=pad_row)
        before = (w.clone(), m.clone(), v.clone())
        for t, k in ((w, 'w'), (m, 'm'), (v, 'v')):
            t[ref['rows']] = ref[k]
        ids, qrow, coef = ar.flat_elements(neg, dneg, qi, pos, dpos)
        keep = (ids >= 0) & (ids != pad_row)
        vals = float(up.double()) * coef[keep].double().unsqueeze(1) * query[qrow[keep]].double()
        p.grad = torch.sparse_coo_tensor(ids[keep].unsqueeze(0), vals, (N, d))
        opt.step()
        st = opt.state[p]
        assert int(ref['K'].sum()) == int(keep.sum()) and ref['rows'].numel() == ids[keep].unique().numel()
        for mine, theirs in ((w, p.data), (m, st['exp_avg']), (v, st['exp_avg_sq'])):
            assert float((mine - theirs).abs().max()) <= 1e-12
        rest = torch.ones(N, dtype=torch.bool)
        rest[ref['rows']] = False
        assert all(torch.equal(t[rest], b[rest]) for t, b in zip((w, m, v), before))          # lazy: other rows keep their state


def _conditioned_case(seed, zero_state, single, d=16):
    """Inputs as the GPU cases condition them: prior exp_avg of the order of g, exp_avg_sq in [0.5, 1.5] x the row's mean g^2,
    weights of order 0.3.  single: every row one element; else a mix of runs of 1 .. ~200 elements across chunk borders."""
    g = torch.Generator().manual_seed(seed)
    N, U = 200, 23
    if single:
        M, n = N, 1
        neg = torch.randperm(N, generator=g).view(M, 1)
        query = torch.randn(M, d, generator=g)
        qi, pos, dpos = None, None, None
        dneg = torch.randn(M, n, generator=g)
    else:
        M, n = 60, 20
        query, qi, neg, pos, dneg, dpos = _step_inputs(g, N, U, d, M, n)
        neg[:, ::2] = torch.randint(0, 6, (M, n // 2), generator=g)
    grad = ar.row_gradients(query, neg, dneg, query_index=qi, pos_ids=pos, dpos=dpos, pad_row=0)
    w = torch.randn(N, d, generator=g) * 0.3
    m, v = torch.zeros(N, d), torch.zeros(N, d)
    if not zero_state:
        scale = torch.ones(N, 1, dtype=torch.float64)
        scale[grad['rows']] = grad['g'].pow(2).mean(1, keepdim=True)
        m = (torch.randn(N, d, generator=g).double() * scale.sqrt()).float()
        v = ((0.5 + torch.rand(N, d, generator=g)).double() * scale).float()
    return dict(query=query, neg_ids=neg, dneg=dneg, query_index=qi, pos_ids=pos, dpos=dpos, pad_row=0), (w, m, v)


def _emulation_ratios(step, betas, zero_state, single, float_betas, chunk=16, lr=0.5):
    kw, (w, m, v) = _conditioned_case(11 + step, zero_state, single)
    hp = dict(lr=lr, betas=betas, eps=1e-8, step=step)
    ref = ar.referee(w, m, v, **kw, **hp)
    rows, w1, m1, v1 = ar.emulate_fp32(w, m, v, **kw, **hp, chunk=chunk, float_betas=float_betas)
    assert np.array_equal(rows, ref['rows'].numpy())
    return ar.bound_ratios(ref, torch.from_numpy(w1), torch.from_numpy(m1), torch.from_numpy(v1)), (ref, v1)


@pytest.mark.parametrize('step', [1, 2, 1000])
def test_bound_admits_fp32_with_the_callers_constants_and_rejects_float32_betas(step):
    """What the bound of adam_referee.tolerances can resolve.  An fp32 emulation of the kernels' arithmetic (sorted order, 16- and
    64-element chunks with partials, one rounding per operation) with 1 - beta and the bias corrections taken from the caller's
    doubles stays within HALF the bound on all three tables, zero and nonzero state, single-element rows and runs across chunk
    borders; the same emulation with the hyper-parameters rounded to fp32 first (1.f - float(0.999) = 0.0009999871, -1.29e-5
    relative) is OUTSIDE it: on the weights of a conditioned nonzero state (the step size is off in one direction on every
    touched row) and on exp_avg_sq of a zero state (off by 1.29e-5 relative where the bound allows ~14 u = 8e-7).
    Nobody widens the bound without this test noticing."""
    betas = (0.9, 0.999)
    for zero_state in (False, True):
        for single in (False, True):
            for chunk in (16, 64):
                r, _ = _emulation_ratios(step, betas, zero_state, single, float_betas=False, chunk=chunk)
                assert max(r) <= 0.5, (zero_state, single, chunk, r)
    r, _ = _emulation_ratios(step, (0.5, 0.9), False, False, float_betas=False)
    assert max(r) <= 0.5, r
    bad_w, _ = _emulation_ratios(step, betas, False, True, float_betas=True)
    assert bad_w[0] > 1.0, bad_w
    bad_v, (ref, v1) = _emulation_ratios(step, betas, True, True, float_betas=True)
    assert bad_v[2] > 1.0, bad_v
    rel = (torch.from_numpy(v1).double() - ref['v']).abs() / ref['v']
    assert 1.2e-5 < float(rel.median()) < 1.4e-5
