"""The forms of the in-place BPR SGD step as the GPU tests run them: each updates ``iw`` / ``uw`` in place and returns
(loss, neg_ids, the coefficients its forward wrote: dpos, dneg, query_grad, pos_score, neg_score).  Shared by
test_gpu_sgd_step.py and the headline-size test of test_gpu_round6.py; ``ra`` is the imported recstudio_amd package."""
import ctypes

import torch


def _coefficients_of(ra, iw0, uw0, n, uid, pos, neg):
    """What the all-sorted form's forward writes on the START tables: the same forward on the same inputs, but a launch of its own
    (the negatives given, not drawn).  test_sgd_step_vs_float64_referee asserts that dpos, dneg and query_grad of this launch
    are bit-equal to what the two-call form's own forward wrote into its kept block, so Stage A of the all-sorted form is fed
    what a step's forward writes, not an assumption."""
    o = ra.ops.fused_forward(iw0, uw0, n, query_index=uid, pos_ids=pos, neg_ids=neg, sampler=ra._native.SAMPLER_GIVEN, want_logp=False,
                             fused_bpr=True, want_query_grad=True)
    return {k: o[k].clone() for k in ('dpos', 'dneg', 'query_grad', 'pos_score', 'neg_score')}


def step_all_sorted(ra, iw, uw, n, lr, uid, pos, sampler, neg, atomics=False):
    iw0, uw0 = iw.clone(), uw.clone()
    kw = {'sampler': sampler} if sampler is not None else {'neg_ids': neg}
    loss, ids = ra.fused.bpr_sgd_step(iw, uw, n, lr, user_ids=uid, pos_ids=pos, in_forward=False, atomics=atomics, **kw)
    return loss.clone(), ids.clone(), _coefficients_of(ra, iw0, uw0, n, uid, pos, ids)


def step_two_calls(ra, iw, uw, n, lr, uid, pos, sampler, neg):
    """The in-forward form as fused._bpr_sgd_step_in_forward issues it -- the argument block of fused._sgd_step_block, then
    rsa_bpr_sgd_prepare and rsa_bpr_sgd_apply on the current stream -- with the block kept: dpos, dneg, query_grad and the scores
    are what THIS step's forward wrote."""
    fused, nat, ops = ra.fused, ra._native, ra.ops
    M = uid.numel()
    kind, kw = fused._sampler_cfg(sampler, neg, M)
    dev = iw.device
    step = torch.full((1,), -float(lr), dtype=torch.float32, device=dev)
    b = fused._sgd_step_block(iw, uw, n, M, kind, sampler, step, neg=neg.contiguous() if kind == nat.SAMPLER_GIVEN else None)
    a = b['args']
    keep = None
    if kind == nat.SAMPLER_POPULAR:
        pop, keep = fused._popular_block(sampler)
        a.pop = ctypes.pointer(pop)
    a.user_ids, a.pos_ids = uid.data_ptr(), pos.data_ptr()
    if kind != nat.SAMPLER_GIVEN:
        fused._reserve_draw(a, kind, sampler, M, n, dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    a.loss_out = loss.data_ptr()
    main = torch.cuda.current_stream(dev)
    a.reduce_scratch = nat.ptr(ops._scratch_for(dev, main.cuda_stream))
    for name in ('rsa_bpr_sgd_prepare', 'rsa_bpr_sgd_apply'):
        rc = getattr(nat.lib(), name)(b['ref'], main.cuda_stream)
        if rc != 0:
            nat.check(rc, name)
    torch.cuda.synchronize()
    del keep
    return loss.clone(), b['neg'].clone(), {k: b[k].clone() for k in ('dpos', 'dneg', 'query_grad', 'pos_score', 'neg_score')}


def step_prefetched(ra, iw, uw, n, lr, uid, pos, sampler, neg):
    stepper = ra.fused.PrefetchedBPRSGD(iw, uw, n, lr, sampler)
    ticket = stepper.prepare(uid, pos)
    loss, ids = stepper.step(ticket)
    torch.cuda.synchronize()
    b = ticket['slot']
    return loss.clone(), ids.clone(), {k: b[k].clone() for k in ('dpos', 'dneg', 'query_grad', 'pos_score', 'neg_score')}


FORMS = {'all-sorted': step_all_sorted, 'two-calls': step_two_calls, 'prefetched': step_prefetched}
