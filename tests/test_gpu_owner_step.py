"""The owner-side sharded training step (rsa_owner.hip) at 2, 3 and 4 owners against the float64 referee of the UNSHARDED step
(tests/owner_referee.py), stage by stage.  One process, one GPU, no collectives: the G owners are played one after the other through
HipBackend -- each with its own state words, its own table block and its own hand-written received segments -- and what the
all-reduces would deliver is a torch sum / max of the owners' tensors.  The (max, rescaled sum, logsumexp) lines of
ShardedItemTable.ssm_step_on_owners are restated in ``_lse``.

Covered because there are several owners: positives owned elsewhere, queries without a slot on an owner, runs of 1 .. 63 elements
and ragged tails, more waves per query than the run has tiles, the merge of (run_max, run_sum, run_acc) across owners, several
received segments with empty ones, dead keys and garbage behind the live counts, the overflow gate, query-grouped segments against
the sort by query, the split calls (forward_parts 1 + 2, finish_parts 1 + 2), determinism.  The shapes are owner_referee.CASES; the
streaming (streams_past_cache, tables over 512 MB) instantiations of the walks are out of scope here.

Every test prints its worst error / bound per stage with the measured transcendental allowance and with none (run with -s).
Measured on an MI355X: torch's fp32 sigmoid (scaled by 1 / n / Q) / exp / log(1 + t) at most 2.4 .. 3.6 / 1.4 / 2.4 u, the allowances
twice that.  Worst error / bound over the cases, with the allowance (and with none): BPR d_slots 0.20 (0.81), dsum_part 0.006, loss
< 0.001, query gradients Stage A 0.019, rows Stage A 0.36 as a gradient block and 0.50 in place (the one rounding of the
read-modify-write), end to end 0.50; SampledSoftmax z 0.056, lse 0.014 (0.022), run_sum 0.009, run_acc 0.015 (0.020), d_slots 0.020
(0.027), rows 0.37 / 0.50, query gradients 0.006 (0.009).  No kernel defect was found.
The two forms of a step (gradient block, in place) share their coefficients bit for bit (asserted) and each is inside Stage A of the
same float64 sums, which is how far they can differ from each other."""
import functools

import pytest
import torch

import owner_referee as orf

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LR = 0.5


@pytest.fixture(scope='module')
def be():
    import recstudio_amd
    recstudio_amd._native.lib()
    from recstudio_amd.shard import HipBackend
    return HipBackend()


@functools.lru_cache(maxsize=None)
def _step(name, dropped=0):
    return orf.make_step(**orf.CASES[name], dropped=dropped, device=DEV)


@functools.lru_cache(maxsize=None)
def _ref(name, loss, use_logq=True):
    return orf.reference(_step(name), loss, LR, use_logq=use_logq)


@functools.lru_cache(maxsize=8)
def _allow(Q, n):
    return orf.allowances(DEV, Q, n)


def _lse(run_max, run_sum, z_pos):
    """shard.py, ssm_step_on_owners: m = max(all-reduce max of run_max, z_pos); s = all-reduce sum of run_sum * exp(run_max - m);
    lse = m + log(s + exp(z_pos - m))"""
    m = torch.maximum(torch.stack(run_max).amax(0), z_pos)
    s = torch.stack([rs * torch.exp(rm - m) for rs, rm in zip(run_sum, run_max)]).sum(0)
    return m + torch.log(s + torch.exp(z_pos - m))


def _owner_args(step, ow, inplace):
    table = ow['table'].clone()
    target = table if inplace else torch.zeros_like(table)
    scale = torch.full((1,), -LR, dtype=torch.float32, device=DEV) if inplace else None
    return table, target, scale


def _pos_scores(be, step):
    return torch.stack([be.pos_scores(ow['table'], step['q_all'], ow['pos_rows']) for ow in step['owners']]).sum(0)


def play_bpr(be, step, inplace, split=False, grouped=None, states=None):
    Q, n, n_seg, stride, q_all = step['Q'], step['n'], step['n_seg'], step['stride'], step['q_all']
    grouped = step['grouped'] if grouped is None else grouped
    pos_score = _pos_scores(be, step)
    run = []
    for o, ow in enumerate(step['owners']):
        st = states[o] if states else be.new_state(DEV)
        table, target, scale = _owner_args(step, ow, inplace)
        qgrad = torch.zeros_like(q_all)
        if split:
            ctx = be.owner_bpr_prepare(st, table, Q, ow['keys'], n_seg, stride, ow['pos_rows'], n, Q, target, scale,
                                       item_pad_row=ow['pad_row'], keys_grouped=grouped)
            ctx = be.owner_bpr_walk(ctx, q_all, pos_score, qgrad)
        else:
            ctx = be.owner_bpr_forward(st, table, q_all, ow['keys'], n_seg, stride, ow['pos_rows'], pos_score, n, Q, target, scale, qgrad,
                                       item_pad_row=ow['pad_row'], keys_grouped=grouped)
        run.append((st, table, target, qgrad, ctx))
    dsum_all = torch.stack([r[4]['dsum_part'] for r in run]).sum(0)
    owners = []
    for st, table, target, qgrad, ctx in run:
        if split:
            be.owner_bpr_finish(ctx, dsum_all, parts=1)
            be.owner_bpr_finish(ctx, dsum_all, parts=2)
        else:
            be.owner_bpr_finish(ctx, dsum_all)
        owners.append(dict(d_slots=ctx['d_slots'], dsum_part=ctx['dsum_part'], loss_part=ctx['loss_part'], qgrad=qgrad, target=target,
                           table=table, step_dropped=int(st['step_dropped']), overflow=int(st['overflow'])))
    return dict(pos_score=pos_score, owners=owners)


def play_ssm(be, step, inplace, use_logq=True, grouped=None, states=None):
    Q, n, n_seg, stride, q_all = step['Q'], step['n'], step['n_seg'], step['stride'], step['q_all']
    grouped = step['grouped'] if grouped is None else grouped
    lq = use_logq and step['logq'] is not None
    z_pos = _pos_scores(be, step)
    if lq:
        z_pos = z_pos - step['logq'][step['pos']]
    run = []
    for o, ow in enumerate(step['owners']):
        st = states[o] if states else be.new_state(DEV)
        table, target, scale = _owner_args(step, ow, inplace)
        ctx = be.owner_ssm_forward(st, table, q_all, ow['keys'], n_seg, stride, ow['pos_rows'], n, Q, target, scale,
                                   logq_rows=ow['logq_rows'] if lq else None, item_pad_row=ow['pad_row'], keys_grouped=grouped)
        run.append((st, table, target, ctx, ctx['d_slots'][:step['slots']].clone()))
    lse = _lse([r[3]['run_max'] for r in run], [r[3]['run_sum'] for r in run], z_pos)
    owners = []
    for st, table, target, ctx, z_slots in run:
        qgrad = torch.zeros_like(q_all)
        be.owner_ssm_finish(ctx, lse, z_pos, qgrad)
        owners.append(dict(z_slots=z_slots, run_max=ctx['run_max'], run_sum=ctx['run_sum'], run_acc=ctx['run_acc'], d_slots=ctx['d_slots'],
                           qgrad=qgrad, target=target, table=table, step_dropped=int(st['step_dropped']), overflow=int(st['overflow'])))
    return dict(z_pos=z_pos, lse=lse, owners=owners)


def _same(a, b, step, keys):
    """bit-equal outputs of two plays (d_slots: the live slots and the positives' coefficients; the rest is never written)"""
    for ow, x, y in zip(step['owners'], a['owners'], b['owners']):
        for k in keys:
            if k == 'z_slots':
                if not torch.equal(x[k][ow['slot']], y[k][ow['slot']]):
                    return False
            elif k == 'd_slots':
                if not (torch.equal(x[k][ow['slot']], y[k][ow['slot']]) and torch.equal(x[k][step['slots']:], y[k][step['slots']:])):
                    return False
            elif not torch.equal(x[k], y[k]):
                return False
    return True


def _report(label, res, res0):
    print(f'{label}: error / bound  ' + '  '.join(f'{k} {v:.3f} ({res0[k]:.3f})' for k, v in res.items()) + '   (in brackets: no allowance)')


def _check_block_form(step, out):
    for ow, oo in zip(step['owners'], out['owners']):
        assert torch.equal(oo['table'], ow['table'])              # the gradient-block form only reads the table
        assert oo['step_dropped'] == 0 and oo['overflow'] == 0


def _check_inplace_form(step, out):
    for ow, oo in zip(step['owners'], out['owners']):
        if ow['pad_row'] >= 0:
            assert torch.equal(oo['target'][ow['pad_row']], ow['table'][ow['pad_row']])
        assert float((oo['target'] - ow['table']).abs().max()) > 1e-6      # the step trained


@pytest.mark.parametrize('name', list(orf.CASES))
def test_bpr_step_on_2_to_4_owners_vs_float64(be, name):
    step, ref = _step(name), _ref(name, 'bpr')
    allow = _allow(step['Q'], step['n'])
    print(f'{name}: torch fp32 sigmoid / exp / log max error {allow["measured"][0]:.2f} / {allow["measured"][1]:.2f} / {allow["measured"][2]:.2f} u, '
          f'allowances {allow["sig"]:.2f} / {allow["exp"]:.2f} / {allow["log"]:.2f} u')
    blk = play_bpr(be, step, False)
    res = orf.judge_bpr(step, ref, blk, allow, False)
    _report(f'{name} BPR gradient block', res, orf.judge_bpr(step, ref, blk, orf.ZERO_ALLOW, False))
    _check_block_form(step, blk)
    assert orf.worst(res) <= 1.0, res
    inp = play_bpr(be, step, True)
    res = orf.judge_bpr(step, ref, inp, allow, True)
    _report(f'{name} BPR in place', res, orf.judge_bpr(step, ref, inp, orf.ZERO_ALLOW, True))
    _check_inplace_form(step, inp)
    assert orf.worst(res) <= 1.0, res
    # the two forms: the same coefficients bit for bit (each is inside Stage A of the same sums, above)
    assert _same(blk, inp, step, ('d_slots', 'dsum_part'))
    # the split calls: forward_parts 1 + 2 and finish_parts 1 + 2 == the one-call step, bit for bit; and a second run
    keys = ('d_slots', 'dsum_part', 'loss_part', 'qgrad', 'target')
    assert _same(inp, play_bpr(be, step, True, split=True), step, keys)
    assert _same(blk, play_bpr(be, step, False, split=True), step, keys)
    assert _same(inp, play_bpr(be, step, True), step, keys)
    if step['grouped']:         # the same segments through the sort by query
        srt = play_bpr(be, step, True, grouped=False)
        res = orf.judge_bpr(step, ref, srt, allow, True)
        _report(f'{name} BPR in place, sorted by query', res, orf.judge_bpr(step, ref, srt, orf.ZERO_ALLOW, True))
        assert orf.worst(res) <= 1.0, res
        assert _same(inp, srt, step, ('d_slots',))              # an element's coefficient does not depend on its place in the run


@pytest.mark.parametrize('sampler', ['popular', 'uniform'])
@pytest.mark.parametrize('name', list(orf.CASES))
def test_sampled_softmax_step_on_2_to_4_owners_vs_float64(be, name, sampler):
    lq = sampler == 'popular'
    step, ref = _step(name), _ref(name, 'ssm', lq)
    allow = _allow(step['Q'], step['n'])
    blk = play_ssm(be, step, False, use_logq=lq)
    res = orf.judge_ssm(step, ref, blk, allow, False)
    _report(f'{name} SSM {sampler} gradient block', res, orf.judge_ssm(step, ref, blk, orf.ZERO_ALLOW, False))
    _check_block_form(step, blk)
    assert orf.worst(res) <= 1.0, res
    inp = play_ssm(be, step, True, use_logq=lq)
    assert _same(blk, inp, step, ('z_slots', 'run_max', 'run_sum', 'run_acc')) and torch.equal(blk['lse'], inp['lse'])
    for a, b in zip(inp['owners'], blk['owners']):       # in place the solo slots keep z: the coefficients are the block form's
        a['d_slots'] = b['d_slots']
    res = orf.judge_ssm(step, ref, inp, allow, True)
    _report(f'{name} SSM {sampler} in place', res, orf.judge_ssm(step, ref, inp, orf.ZERO_ALLOW, True))
    _check_inplace_form(step, inp)
    assert orf.worst(res) <= 1.0, res
    keys = ('z_slots', 'run_max', 'run_sum', 'run_acc', 'qgrad', 'target')
    assert _same(inp, play_ssm(be, step, True, use_logq=lq), step, keys)
    if step['grouped'] and lq:
        srt = play_ssm(be, step, True, use_logq=lq, grouped=False)
        assert _same(inp, srt, step, ('z_slots', 'run_max'))
        for a, b in zip(srt['owners'], blk['owners']):
            a['d_slots'] = None                            # (lse may differ in its last bit: the block form's d is not this run's)
        res = orf.judge_ssm(step, ref, srt, allow, True)
        _report(f'{name} SSM {sampler} in place, sorted by query', res, orf.judge_ssm(step, ref, srt, orf.ZERO_ALLOW, True))
        assert orf.worst(res) <= 1.0, res


@pytest.mark.parametrize('loss', ['bpr', 'ssm'])
@pytest.mark.parametrize('name', ['shared_small', 'mix_ragged'])
def test_gated_step_changes_nothing_and_counts(be, name, loss):
    """Header word 1 non-zero on ONE segment of every owner: tables and qgrad_all bit-unchanged, step_dropped = the sum of the
    header words, the sticky overflow word accumulates over two steps."""
    step = _step(name, 3)
    play = play_bpr if loss == 'bpr' else play_ssm
    states = [be.new_state(DEV) for _ in step['owners']]
    for k in (1, 2):
        out = play(be, step, True, states=states)
        assert orf.judge_gated(step, out) == 0
        assert all(oo['step_dropped'] == 3 and oo['overflow'] == 3 * k for oo in out['owners'])
    out = play(be, step, False, states=states)             # a gradient block stays zero
    assert all(not bool(oo['target'].any()) and not bool(oo['qgrad'].any()) and oo['overflow'] == 9 for oo in out['owners'])
