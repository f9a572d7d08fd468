"""CPU: the float64 referee of the Adagrad row update (tests/adagrad_referee.py) is torch.optim.Adagrad's own arithmetic on sparse AND
on dense gradients; the error bound the GPU tests apply (adagrad_referee.tolerances) admits an fp32 emulation of the kernels'
arithmetic and rejects every seeded mistake; and the host side of the feature that runs without a GPU: the argument block's
validation and ``fit``'s choice of the step."""
import ctypes

import numpy as np
import pytest
import torch

import adagrad_referee as gr
import adam_referee as ar
from test_adam_referee import _step_inputs


# ------------------------------------------------------------------------------------------------------- the referee is torch's rule
@pytest.mark.parametrize('sparse', [True, False], ids=['sparse-grad', 'dense-grad'])
@pytest.mark.parametrize('pad_row', [0, -1])
def test_referee_equals_torch_adagrad_in_float64(sparse, pad_row):
    """Six steps with repeating rows (rows 30 .. 39 only from step 3 on, so that states of different ages coexist; rows 40 .. 47
    never), lr_decay > 0,
    a nonzero initial_accumulator_value: weight and state_sum of the referee == torch.optim.Adagrad on float64 parameters fed the
    gradient of the same elements -- as a COO tensor (the sparse branch: coalesce, square the coalesced values) and as a dense
    tensor (zero rows for everything else) -- to 1e-12 absolute (inputs of order 1).  Rows outside a step: bit-unchanged in the
    referee's tables AND in torch's, dense branch included (0 / (sqrt(s) + eps) = 0)."""
    g = torch.Generator().manual_seed(3)
    N, U, d, M, n, lr, lr_decay, eps, acc0 = 48, 17, 8, 30, 10, 0.05, 0.3, 1e-10, 0.1
    w = torch.randn(N, d, generator=g)
    p = torch.nn.Parameter(w.double().clone())
    opt = torch.optim.Adagrad([p], lr=lr, lr_decay=lr_decay, initial_accumulator_value=acc0, eps=eps)
    w, s = w.double(), torch.full((N, d), acc0, dtype=torch.float64)
    up = torch.tensor([0.37])
    for step in range(1, 7):
        query, qi, neg, pos, dneg, dpos = _step_inputs(g, 30 if step < 3 else 40, U, d, M, n)
        ref = gr.referee(w, s, query, neg, dneg, lr=lr, lr_decay=lr_decay, eps=eps, step=step, query_index=qi, pos_ids=pos, dpos=dpos,
                         upstream=up, pad_row=pad_row)
        before = (w.clone(), s.clone())
        w[ref['rows']], s[ref['rows']] = ref['w'], ref['s']
        ids, qrow, coef = ar.flat_elements(neg, dneg, qi, pos, dpos)
        keep = (ids >= 0) & (ids != pad_row)
        vals = float(up.double()) * coef[keep].double().unsqueeze(1) * query[qrow[keep]].double()
        grad = torch.sparse_coo_tensor(ids[keep].unsqueeze(0), vals, (N, d))
        p.grad = grad if sparse else grad.to_dense()
        theirs_before = (p.data.clone(), opt.state[p]['sum'].clone())
        opt.step()
        assert int(opt.state[p]['step']) == step and step * lr_decay > 0
        for mine, theirs in ((w, p.data), (s, opt.state[p]['sum'])):
            assert float((mine - theirs).abs().max()) <= 1e-12
        assert ref['rows'].numel() == ids[keep].unique().numel() < N
        assert gr.untouched_equal(ref, before, (w, s))
        assert gr.untouched_equal(ref, theirs_before, (p.data, opt.state[p]['sum']))


# ------------------------------------------------------------------------------------- what the bound admits and what it rejects
def _conditioned_case(seed, zero_state, single, d=16):
    """Inputs as the GPU cases condition them: prior state_sum in [0.5, 1.5] x the row's mean g^2 (so that an error in g reaches
    the weights: with a zero state at step 1, g / sqrt(g^2) = sign(g) and it cancels), weights of order 0.3.  single: every row
    one element; else a mix of runs of 1 .. ~200 elements across chunk borders.  Untouched rows carry a live state of order 1."""
    g = torch.Generator().manual_seed(seed)
    N, U = 200, 23
    if single:
        M, n = N - 20, 1
        neg = torch.randperm(N, generator=g)[:M].view(M, 1)
        query = torch.randn(M, d, generator=g)
        qi, pos, dpos = None, None, None
        dneg = torch.randn(M, n, generator=g)
    else:
        M, n = 60, 20
        query, qi, neg, pos, dneg, dpos = _step_inputs(g, N - 20, U, d, M, n)
        neg[:, ::2] = torch.randint(0, 6, (M, n // 2), generator=g)
    grad = ar.row_gradients(query, neg, dneg, query_index=qi, pos_ids=pos, dpos=dpos, pad_row=0)
    w = torch.randn(N, d, generator=g) * 0.3
    s = torch.zeros(N, d)
    if not zero_state:
        scale = torch.ones(N, 1, dtype=torch.float64)
        scale[grad['rows']] = grad['g'].pow(2).mean(1, keepdim=True)
        s = ((0.5 + torch.rand(N, d, generator=g)).double() * scale).float()
    return dict(query=query, neg_ids=neg, dneg=dneg, query_index=qi, pos_ids=pos, dpos=dpos, pad_row=0), (w, s)


HP = dict(lr=0.5, lr_decay=0.25, eps=1e-10)


def _ratios(step, zero_state, single, chunk=16, hp=HP, **emu):
    kw, (w, s) = _conditioned_case(11 + step, zero_state, single)
    ref = gr.referee(w, s, **kw, **hp, step=step)
    rows, w1, s1 = gr.emulate_fp32(w, s, **kw, **hp, step=step, chunk=chunk, **emu)
    assert np.array_equal(rows, ref['rows'].numpy())
    return gr.bound_ratios(ref, torch.from_numpy(w1), torch.from_numpy(s1)), ref


@pytest.mark.parametrize('step', [1, 2, 1000])
def test_bound_admits_the_fp32_emulation(step):
    """An fp32 emulation of the kernels' arithmetic (sorted order, 16- and 64-element chunks with partials, one rounding per
    operation, the two fused multiply-adds) stays within HALF the bound on both tables: zero and conditioned state, single-element
    rows and runs across chunk borders, torch's eps and a large one."""
    for zero_state in (False, True):
        for single in (False, True):
            for chunk in (16, 64):
                for hp in (HP, dict(HP, eps=1e-2, lr_decay=0.0)):
                    r, _ = _ratios(step, zero_state, single, chunk=chunk, hp=hp)
                    assert max(r) <= 0.5, (zero_state, single, chunk, hp, r)


@pytest.mark.parametrize('step', [2, 1000])
def test_bound_rejects_every_seeded_mistake(step):
    """Each mistake leaves a tolerance on the conditioned state (index 0: weight, 1: state_sum); nobody widens the bound without
    this test noticing."""
    # squares summed per element instead of the squared row sum: the state of every row with more than one element
    r, ref = _ratios(step, False, False, mistake='per_element_squares')
    assert int(ref['K'].max()) > 1 and r[1] > 1.0, r
    ok, _ = _ratios(step, False, True, mistake='per_element_squares')          # (one element per row: the two are the same number)
    assert max(ok) <= 0.5, ok
    # the division taken with the old s: the state is right, the weights are not
    r, _ = _ratios(step, False, True, mistake='old_state')
    assert r[0] > 1.0 and r[1] <= 0.5, r
    # eps inside the root (at an eps that can be told from 0; the correct arithmetic at that eps passes above)
    big_eps = dict(HP, eps=1e-2)
    assert max(_ratios(step, False, True, hp=big_eps)[0]) <= 0.5
    r, _ = _ratios(step, False, True, hp=big_eps, mistake='eps_in_root')
    assert r[0] > 1.0 and r[1] <= 0.5, r
    # lr_decay ignored (step > 1)
    r, _ = _ratios(step, False, True, mistake='no_lr_decay')
    assert r[0] > 1.0 and r[1] <= 0.5, r
    # a run's last element dropped: g is wrong on that row, in both tables
    kw, _ = _conditioned_case(11 + step, False, False)
    grad = ar.row_gradients(kw['query'], kw['neg_ids'], kw['dneg'], query_index=kw['query_index'], pos_ids=kw['pos_ids'], dpos=kw['dpos'])
    victim = int(grad['rows'][int(grad['K'].argmax())])
    for chunk in (16, 64):
        r, _ = _ratios(step, False, False, chunk=chunk, drop_element_of=victim)
        assert r[0] > 1.0 and r[1] > 1.0, (chunk, r)
        # a chunk partial scaled (only runs of more than one segment have partials)
        r, _ = _ratios(step, False, False, chunk=chunk, partial_scale=1.01)
        assert r[0] > 1.0 and r[1] > 1.0, (chunk, r)


def test_zero_state_at_step_1_judges_the_state():
    """With s = 0 at step 1, w' = w - clr sign(g) (up to eps): an error in g cancels in the weights and shows in the state alone --
    why the cases with a zero state are there, and why the others condition the state."""
    kw, _ = _conditioned_case(12, True, False)
    grad = ar.row_gradients(kw['query'], kw['neg_ids'], kw['dneg'], query_index=kw['query_index'], pos_ids=kw['pos_ids'], dpos=kw['dpos'])
    victim = int(grad['rows'][int(grad['K'].argmax())])
    r, _ = _ratios(1, True, False, drop_element_of=victim)
    assert r[1] > 1.0, r


def test_an_untouched_rows_state_must_not_change():
    """The seventh mistake: the update itself within the bound, but one row outside the step with its state_sum (or weight)
    rewritten -- even by one ulp."""
    kw, (w, s) = _conditioned_case(13, False, False)
    ref = gr.referee(w, s, **kw, **HP, step=2)
    rows, w1, s1 = gr.emulate_fp32(w, s, **kw, **HP, step=2)
    got_w, got_s = w.clone(), s.clone()
    got_w[torch.from_numpy(rows)], got_s[torch.from_numpy(rows)] = torch.from_numpy(w1), torch.from_numpy(s1)
    assert gr.untouched_equal(ref, (w, s), (got_w, got_s)) and max(gr.bound_ratios(ref, got_w[ref['rows']], got_s[ref['rows']])) <= 0.5
    rest = torch.ones(w.shape[0], dtype=torch.bool)
    rest[ref['rows']] = False
    victims = (int(rest.nonzero()[0]), int(rest.nonzero()[-1]))          # the padding row (it has elements) and a row nobody names
    assert victims[0] == 0 and victims[1] >= 180 and float(s[victims[1]].abs().min()) > 0
    for victim in victims:
        for table in (1, 0):
            bad = [got_w.clone(), got_s.clone()]
            bad[table][victim, 3] = torch.nextafter(bad[table][victim, 3], torch.tensor(float('inf')))
            assert not gr.untouched_equal(ref, (w, s), bad)
    assert gr.untouched_equal(ref, (w, s), (got_w, got_s))
    # row 0 is the padding row here: it has elements (ids 0 .. 5 are hot) and stays out of the step
    assert int((kw['neg_ids'] == 0).sum()) > 10 and not bool((ref['rows'] == 0).any())


# ------------------------------------------------------------------------------------------------ the argument block, without a GPU
@pytest.fixture(scope='module')
def nat():
    import os
    from recstudio_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def _block(nat, **fields):
    """A block that passes every check before the rule's (fake non-null pointers: validation happens before any HIP call and
    dereferences nothing), n_queries = 0 so that a block that passes returns before any launch."""
    a = nat.RowsUpdateArgs()
    a.dim, a.num_neg, a.n_items, a.n_queries = 64, 8, 100, 0
    for k, v in fields.items():
        setattr(a, k, v)
    return a


ENTRIES = ('rsa_rows_update_sorted', 'rsa_rows_update_presorted')
FAKE = 4096


@pytest.mark.parametrize('entry', ENTRIES)
def test_adagrad_block_is_validated_before_any_hip_call(nat, entry):
    lib = nat.lib()
    fn = getattr(lib, entry)
    good = dict(rule=nat.ROWS_ADAGRAD, state_sum=FAKE, lr=0.01, lr_decay=0.0, eps=1e-10, step=1)

    def verdict(**change):
        a = _block(nat, **dict(good, **change))
        rc = fn(ctypes.byref(a), None)
        return rc, lib.rsa_last_error().decode()

    assert verdict()[0] == 0                                              # (n_queries = 0: accepted, nothing to do)
    assert verdict(lr_decay=0.5, eps=0.0, step=7)[0] == 0
    for change, words in ((dict(state_sum=None), 'Adagrad needs state_sum'), (dict(step=0), 'step >= 1'), (dict(eps=-1e-10), 'eps >= 0'),
                          (dict(lr_decay=-0.1), 'lr_decay >= 0'), (dict(exp_avg=FAKE), 'no exp_avg'),
                          (dict(exp_avg_sq=FAKE), 'no exp_avg'), (dict(exp_avg=FAKE, exp_avg_sq=FAKE), 'no exp_avg'),
                          (dict(rule=2), 'unknown rule 2'), (dict(rule=-1), 'unknown rule -1')):
        rc, msg = verdict(**change)
        assert rc == -1 and msg.startswith(entry + ':') and words in msg, (change, msg)
    with pytest.raises(nat.NativeError, match=entry + ': Adagrad needs state_sum'):
        nat.check(verdict(state_sum=None)[0], entry)


@pytest.mark.parametrize('entry', ENTRIES)
def test_rule_0_and_shorter_blocks_keep_todays_verdicts(nat, entry):
    """rule = 0 is the block as it was: accumulate, or lazy Adam by exp_avg, with check_adam's verdicts; a block cut before the new
    fields (an older caller's: whatever lies behind its end is not read) passes the same checks."""
    lib = nat.lib()
    fn = getattr(lib, entry)
    assert nat.RowsUpdateArgs.state_sum.offset == nat.RowsUpdateArgs.workspace_bytes.offset + 8
    assert [f[0] for f in nat.RowsUpdateArgs._fields_[-4:]] == ['state_sum', 'lr_decay', 'rule', '_pad2']
    assert lib.rsa_abi_version() == 13
    adam = dict(exp_avg=FAKE, exp_avg_sq=FAKE, lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, step=1)
    for cut in (False, True):
        junk = dict(rule=7, state_sum=FAKE, lr_decay=-1.0) if cut else {}           # behind the end of a cut block: ignored
        for fields, want in (({}, None), (adam, None), (dict(adam, exp_avg_sq=None), 'bad optimizer state'),
                             (dict(adam, step=0), 'bad optimizer state'), (dict(adam, beta2=1.5), 'bad optimizer state')):
            a = _block(nat, **fields, **junk)
            if cut:
                a.size = nat.RowsUpdateArgs.state_sum.offset
            rc = fn(ctypes.byref(a), None)
            if want is None:
                assert rc == 0, lib.rsa_last_error()
            else:
                assert rc == -1 and lib.rsa_last_error().decode().startswith(entry + ': ' + want)
    a = _block(nat, rule=7)                                                          # the same junk INSIDE the block is an error
    assert fn(ctypes.byref(a), None) == -1 and b'unknown rule 7' in lib.rsa_last_error()
    # rule 0 does not look at state_sum (it is not this rule's field)
    assert fn(ctypes.byref(_block(nat, state_sum=FAKE)), None) == 0


# ------------------------------------------------------------------------------------------------------------------ fit's choice
def test_fit_runs_the_learners_rule_in_the_kernels():
    from recstudio_amd.fused import BPRAdagradStep, BPRSGDStep, FusedBPRAdagrad
    from test_fit_host import stock_model
    step = stock_model()._fused_optimizer_step({'fused_optimizer': 'learner', 'learner': 'adagrad'})
    assert type(step) is BPRAdagradStep and type(step.opt) is FusedBPRAdagrad and step.stepper is None
    # torch.optim.Adagrad's defaults around the configured rate; state = the two state_sum tables
    opt = step.opt
    assert (opt.lr, opt.lr_decay, opt.eps, opt.t) == (0.001, 0.0, 1e-10, 0) and sorted(opt.state) == ['is', 'us']
    assert opt.state['is'].shape == (11, 64) and opt.state['us'].shape == (7, 64) and not opt.state['is'].any()
    step.set_lr(0.25)                                                     # the scheduler's rate reaches the kernel's argument
    assert opt.lr == 0.25 and opt._hp()['lr'] == 0.25
    assert type(stock_model()._fused_optimizer_step({'fused_optimizer': 'learner', 'learner': 'Adagrad', 'learning_rate': 0.5}).opt.lr) is float
    # look-ahead is opt-in, by the rule's own name
    ahead = stock_model()._fused_optimizer_step({'fused_optimizer': 'learner', 'learner': 'adagrad', 'fused_prefetch': 'adagrad'})
    assert ahead.stepper is ahead
    for other in (True, 'adam', False):
        s = stock_model()._fused_optimizer_step({'fused_optimizer': 'learner', 'learner': 'adagrad', 'fused_prefetch': other})
        assert s.stepper is None
    # a nonzero initial accumulator fills both tables
    filled = FusedBPRAdagrad(torch.zeros(5, 64), torch.zeros(3, 64), initial_accumulator_value=0.1)
    assert float(filled.state['is'].min()) == float(filled.state['us'].max()) == float(torch.tensor(0.1))
    with pytest.raises(NotImplementedError, match='64, 128 or 256'):
        FusedBPRAdagrad(torch.zeros(5, 32), torch.zeros(3, 32))
    with pytest.raises(ValueError, match='>= 0'):
        FusedBPRAdagrad(torch.zeros(5, 64), torch.zeros(3, 64), lr_decay=-1.0)
    # 'sgd' under 'learner' is the SGD step (without its look-ahead here: that one opens a side stream)
    sgd = stock_model()._fused_optimizer_step({'fused_optimizer': 'learner', 'learner': 'sgd', 'fused_prefetch': False})
    assert type(sgd) is BPRSGDStep and sgd.stepper is None and sgd.lr == 0.001


def test_fit_learner_setting_refuses_what_it_does_not_cover():
    from test_fit_host import MyBPR, stock_model
    for learner in ('adam', 'rmsprop', 'adamw'):
        with pytest.raises(NotImplementedError, match="'sgd' and 'adagrad'"):
            stock_model()._fused_optimizer_step({'fused_optimizer': 'learner', 'learner': learner})
    with pytest.raises(NotImplementedError, match="'sgd' and 'adagrad'"):           # the model's own default learner: adam
        stock_model()._fused_optimizer_step({'fused_optimizer': 'learner'})
    # the stock-configuration conditions are the existing ones, and come first
    with pytest.raises(NotImplementedError, match='stock BPR two-tower'):
        stock_model(loss_fn=MyBPR())._fused_optimizer_step({'fused_optimizer': 'learner', 'learner': 'adagrad'})
    with pytest.raises(NotImplementedError, match='stock BPR two-tower'):
        stock_model()._fused_optimizer_step({'fused_optimizer': 'learner', 'learner': 'adagrad', 'weight_decay': 0.01})
    # an unknown value names all three
    with pytest.raises(ValueError, match="'sgd' or 'adam', or 'learner'"):
        stock_model()._fused_optimizer_step({'fused_optimizer': 'adagrad'})
