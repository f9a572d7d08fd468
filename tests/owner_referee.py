"""Float64 referee of the OWNER-SIDE sharded training step (rsa_owner.hip: rsa_shard_pos_score, rsa_shard_owner_bpr_forward /
_finish, rsa_shard_owner_ssm_forward / _finish) at 2-4 owners, the bounds a correct fp32 implementation stays inside, and an fp32
emulation of the owner protocol with the mistakes the bounds must catch.  Test code only: nothing here imports recstudio_amd.
Runs on whatever device the step's tensors live on.

The step (unsharded): item table W [N, d] (row 0 the padding row: it receives no update), tower rows q_all [Q = G B, d], one
positive and n negatives per query, all gradients from the PRE-step table:

    BPR  (loss_func.py:55-59)   x_j = s_j - s_pos      d_j = sigmoid(x_j) / (n Q)    dpos = -sum_j d_j     loss = mean softplus(x)
    SSM  (loss_func.py:80-90)   z = s - log q(item)    lse = logsumexp(z_pos, z_1 .. z_n)
                                d_j = exp(z_j - lse) / Q     dpos = (exp(z_pos - lse) - 1) / Q              loss = mean (lse - z_pos)
    qgrad[q] = dpos W[pos] + sum_j d_j W[neg_j]        grad[id] = sum over elements on id of d_e q_all[query_e]     W' = W - lr grad

Sharded: owner(id) / local row follow RowShardPlan ('block': id // rows_per_shard, id - owner * rows_per_shard; 'interleaved':
id % G, id // G -- restated here, pinned against RowShardPlan by test_owner_referee.py).  Every owner receives n_seg = G * banks
segments of stride = SHARD_HDR + cap words: header {live, dropped}, keys ``query << 32 | local row``, garbage behind ``live``.
``make_step`` writes those segments by hand and plants the cases that exist only because there are several owners.

A DEAD key has a row >= n_rows AND a query >= Q: both sorts drop it.  Keys that are bad in ONE half only are outside the kernels'
contract (the router writes none; the walk clamps such a row to the last one, the apply pass would index the query block with the
bad query) and are not planted.

Bounds (u = 2^-24; ``allow`` = the measured error of an fp32 transcendental in units of u x its result, see ``allowances``):

Stage A -- the update arithmetic given the kernel's OWN fp32 coefficients d_slots (sgd_referee's Stage A):
    rows    |T32 - (T + scale g)| <= |scale| (K + 2) u A + 2u |T'|       K = elements on the row, A = sum |d_e q_e|
    qgrad   (BPR) |sum_o qg_o - qg| <= sum_o (K_o + 3) u A_o             K_o = the query's elements on owner o (+ its positive)
Stage B -- the coefficients against float64 scores of the pre-step table (sgd_referee's Stage B for BPR):
    score   e_s = (d + 1) u sum_i |q_i w_i|
    BPR     |d32 - d| <= d ((1 - sig)(e_x + 2u |x|) + allow u),  e_x = e_neg + e_pos;   dsum: the sum of those + (K - 1) u |dsum|
            loss share: sum_e (sig e_x + (allow + 4) u softplus) / (n Q) + E u sum (any order of E terms)
    SSM     z: e_s + 2u |z| + u |log q|;   run_max == max of the kernel's own z, bit for bit;  run_sum, run_acc against
            sum exp(z64 - run_max32) [row]: every term by rel_K = (2K + 20) u  (two roundings per online-softmax step, the lane
            and wave merges) + (K + 9) allow u (its own exp and at most K rescales) + 4u range(z) (the hardware exp's argument
            error 2u |x|, telescoped over the rescales), + its z error;  lse: the softmax-weighted z errors + rel_K + the restated
            reduction's few fp32 operations;  d_j: d (tol_z + tol_lse + 2u |z - lse| + allow u);  qgrad: carried through.
No fitted constants.
"""
import torch

import adam_referee as ar
import sort_referee as sf

U32 = ar.U32
HDR = sf.SHARD_HDR
MISTAKES = ('local_dsum', 'merge_without_rescale', 'acc_without_rescale', 'pos_by_non_owner', 'mean_over_local_batch',
            'solo_twice', 'ragged_tail_dropped', 'padding_row_updated', 'gate_ignored', 'slack_is_live')

# The shapes of the GPU test (tests/test_gpu_owner_step.py); slots / Q / 64 picks owner_walk_geometry's class.
CASES = {
    # almost every row shared; 1 wave per query; single-workgroup sorts (slots <= 4096); runs of ~32 elements
    'shared_small': dict(G=2, B=8, n=64, rows_per_shard=97, d=64, layout='block', grouped=False, banks=2, seed=1),
    # a mix; 2 waves per query (class 3-7); multi-tile radix sort (slots > 4096); n = 200: ragged runs everywhere
    'mix_ragged': dict(G=3, B=16, n=200, rows_per_shard=2003, d=128, layout='interleaved', grouped=True, banks=2, cap=2100, seed=2),
    # almost every row solo; 4 waves per query (class >= 8) over runs of ~2 tiles: partial waves idle
    'solo_idle_waves': dict(G=4, B=8, n=512, rows_per_shard=40_009, d=256, layout='block', grouped=True, banks=2, cap=2050, seed=3),
    # no padding row; long runs (n = 1024), 4 waves per query all busy
    'no_pad_long': dict(G=2, B=40, n=1024, rows_per_shard=2003, d=64, layout='interleaved', grouped=False, banks=2, pad=False, seed=4),
    # three owners, shared rows, ragged, ungrouped
    'shared_ragged': dict(G=3, B=8, n=200, rows_per_shard=97, d=128, layout='block', grouped=False, banks=3, seed=5),
}


# ------------------------------------------------------------------------------------------------------------------- the plan
def n_items_of(G, rows_per_shard):
    """One row short of G full shards: the last block (and the last interleaved residues) is a row shorter."""
    return G * rows_per_shard - 1


def owner_of(ids, N, G, layout):
    if layout == 'interleaved':
        return ids.clamp(min=0) % G
    rps = (N + G - 1) // G
    return (ids // rps).clamp(0, G - 1)


def local_of(ids, N, G, layout):
    if layout == 'interleaved':
        return ids.clamp(min=0) // G
    rps = (N + G - 1) // G
    return (ids - owner_of(ids, N, G, layout) * rps).clamp(min=0)


def n_local(o, N, G, layout):
    if layout == 'interleaved':
        return max(0, (N - o + G - 1) // G)
    rps = (N + G - 1) // G
    lo = min(N, o * rps)
    return min(N, lo + rps) - lo


def global_id(o, local, N, G, layout):
    return local * G + o if layout == 'interleaved' else local + o * ((N + G - 1) // G)


def take(full, o, N, G, layout):
    if layout == 'interleaved':
        return full[o::G]
    rps = (N + G - 1) // G
    return full[o * rps:min(N, (o + 1) * rps)]


def pack_keys(query, row):
    return (query.to(torch.int64) << 32) | row.to(torch.int64)


# -------------------------------------------------------------------------------------------------------------- the step builder
def make_step(G, B, n, rows_per_shard, d, seed, layout, grouped, banks=2, cap=None, pad=True, dropped=0, popular=True,
              device='cpu'):
    """-> dict: the unsharded step (W, q_all, pos [Q], neg [Q, n], logq [N] or None) and per owner ``owners[o]`` = dict(table
    [n_rows, d], keys [n_seg * stride] int64, pos_rows [Q] (-1: owned elsewhere), pad_row, logq_rows, and the bookkeeping of the
    real elements: slot, eq (query), ej (column), rows (local row), ids (global)).  ``dropped``: header word 1 of ONE segment of every owner."""
    g = torch.Generator().manual_seed(seed)
    Q, N = G * B, n_items_of(G, rows_per_shard)
    W = torch.randn(N, d, generator=g) * 0.3
    W[0] = 0
    q_all = torch.randn(Q, d, generator=g) * 0.3
    pos = torch.randint(1, N, (Q,), generator=g)
    neg = torch.randint(1, N, (Q, n), generator=g)
    nl = [n_local(o, N, G, layout) for o in range(G)]
    # planted: query 0 entirely on owner 0 (empty runs elsewhere); query 1: ONE element on owner 1, the rest on owner 0
    neg[0] = global_id(0, torch.randint(1, nl[0], (n,), generator=g), N, G, layout)
    neg[1] = global_id(0, torch.randint(1, nl[0], (n,), generator=g), N, G, layout)
    neg[1, 0] = global_id(1, torch.randint(1, nl[1], (1,), generator=g), N, G, layout)
    # negatives equal to the query's own positive and to other queries' positives (shared rows); the padding row
    neg[2, :3] = pos[2]
    neg[2, 3], neg[2, 4] = pos[3], pos[4]
    neg[3, :2] = 0
    logq = None
    if popular:
        cnt = (torch.rand(N, generator=g) ** 3 * 50).floor() + 1
        logq = torch.log(cnt / cnt.sum()).to(torch.float32)
    own, loc = owner_of(neg, N, G, layout), local_of(neg, N, G, layout)
    qi = torch.arange(Q).view(Q, 1).expand(Q, n)
    ji = torch.arange(n).view(1, n).expand(Q, n)
    n_seg = G * banks
    plans, longest = [], 0
    for o in range(G):
        m = own == o
        eq, ej, er = qi[m], ji[m], loc[m]
        src = eq // B
        nb = torch.where(src == 0, max(1, banks - 1), banks)          # source 0 never uses its last bank: a live = 0 segment
        seg = src * banks + (eq % nb if grouped else (eq + ej) % nb)
        per = []
        for s in range(n_seg):
            idx = (seg == s).nonzero().view(-1)                        # (q, j) order: every query one contiguous run
            if not grouped and idx.numel():
                idx = idx[torch.randperm(idx.numel(), generator=g)]
            dead_at = []
            if s == n_seg - 1 and idx.numel() > 2:                     # dead keys in front, at a run boundary and behind
                qs = eq[idx]
                change = (qs[1:] != qs[:-1]).nonzero().view(-1)
                mid = int(change[0]) + 1 if change.numel() else 1
                dead_at = [0, mid, idx.numel()]
            per.append((idx, dead_at))
            longest = max(longest, idx.numel() + len(dead_at))
        plans.append((eq, ej, er, per))
    cap = longest + 5 if cap is None else int(cap)
    assert cap >= longest + 1, f'cap {cap} < longest segment {longest} + slack'
    stride = HDR + cap
    owners = []
    for o in range(G):
        eq, ej, er, per = plans[o]
        n_rows = nl[o]
        keys = torch.empty(n_seg, stride, dtype=torch.int64)
        # the slack: keys that LOOK live (a real query, a real row)
        keys[:, HDR:] = pack_keys(torch.randint(0, Q, (n_seg, cap), generator=g), torch.randint(1, n_rows, (n_seg, cap), generator=g))
        slot = torch.empty(eq.numel(), dtype=torch.int64)
        n_dead = 0
        for s, (idx, dead_at) in enumerate(per):
            k = pack_keys(eq[idx], er[idx])
            at = torch.arange(idx.numel())
            for t, p in enumerate(dead_at):
                dead = pack_keys(torch.tensor([Q + 1, 2 ** 31 - 1, Q][t]), torch.tensor([n_rows + 9, 2 ** 32 - 1, n_rows][t]))
                k = torch.cat([k[:p + t], dead.view(1), k[p + t:]])
                at = at + (at >= p + t).long()
                n_dead += 1
            keys[s, 0], keys[s, 1] = k.numel(), 0
            keys[s, HDR:HDR + k.numel()] = k
            slot[idx] = s * stride + HDR + at
        if dropped:
            keys[min(1, n_seg - 1), 1] = int(dropped)
        po = owner_of(pos, N, G, layout) == o
        pos_rows = torch.where(po, local_of(pos, N, G, layout), torch.full_like(pos, -1))
        owners.append(dict(n_rows=n_rows, keys=keys.reshape(-1).to(device), pos_rows=pos_rows.to(device),
                           pad_row=0 if (pad and o == 0) else -1, table=take(W, o, N, G, layout).contiguous().to(device),
                           logq_rows=None if logq is None else take(logq, o, N, G, layout).contiguous().to(device),
                           slot=slot.to(device), eq=eq.to(device), ej=ej.to(device), rows=er.to(device),
                           ids=global_id(o, er, N, G, layout).to(device), n_dead=n_dead))
    return dict(G=G, B=B, n=n, Q=Q, d=d, N=N, layout=layout, grouped=grouped, banks=banks, cap=cap, stride=stride, n_seg=n_seg,
                slots=n_seg * stride, pad=pad, W=W.to(device), q_all=q_all.to(device), pos=pos.to(device), neg=neg.to(device),
                logq=None if logq is None else logq.to(device), owners=owners, dropped=int(dropped) * G if dropped else 0)


def planted(step):
    """Counts of the planted cases, read back from the finished step."""
    Q, stride = step['Q'], step['stride']
    out = dict(empty_runs=0, one_element_runs=0, ragged_runs=0, live0_segments=0, dead_keys=0, shared_pos_rows=0, pad_negatives=0,
               solo_row_foreign_pos=0)
    pos_cnt = torch.bincount(step['pos'], minlength=step['N'])
    for o, ow in enumerate(step['owners']):
        run = torch.bincount(ow['eq'], minlength=Q)
        out['empty_runs'] += int((run == 0).sum())
        out['one_element_runs'] += int((run == 1).sum())
        out['ragged_runs'] += int(((run % 64) != 0).sum())
        out['live0_segments'] += int((ow['keys'].view(-1, stride)[:, 0] == 0).sum())
        out['dead_keys'] += ow['n_dead']
        out['shared_pos_rows'] += int((pos_cnt[ow['ids']] > 0).sum())
        out['pad_negatives'] += int((ow['ids'] == 0).sum())
        # a row ONE element touches here while that element's query has its positive on another owner
        touch = torch.bincount(ow['rows'], minlength=ow['n_rows']) + torch.bincount(ow['pos_rows'][ow['pos_rows'] >= 0],
                                                                                  minlength=ow['n_rows'])
        out['solo_row_foreign_pos'] += int(((touch[ow['rows']] == 1) & (ow['pos_rows'][ow['eq']] < 0)).sum())
    return out


# ------------------------------------------------------------------------------------------------------------ the float64 referee
def reference(step, loss, lr, use_logq=True):
    """The unsharded float64 step -> dict; per-owner intermediates under ``owners[o]``.  ``loss``: 'bpr' | 'ssm'."""
    W, q_all, pos, neg = step['W'], step['q_all'], step['pos'], step['neg']
    Q, n, d, N, G = step['Q'], step['n'], step['d'], step['N'], step['G']
    q64 = q_all.double()
    wp = W[pos].double()
    s_pos = (q64 * wp).sum(-1)
    e_pos = (d + 1) * U32 * (q64 * wp).abs().sum(-1)
    s_neg = torch.empty(Q, n, dtype=torch.float64, device=W.device)
    e_neg = torch.empty_like(s_neg)
    for lo in range(0, Q, 16):
        t = q64[lo:lo + 16].unsqueeze(1) * W[neg[lo:lo + 16]].double()
        s_neg[lo:lo + 16], e_neg[lo:lo + 16] = t.sum(-1), (d + 1) * U32 * t.abs().sum(-1)
    logq = step['logq'] if (use_logq and loss == 'ssm') else None
    ref = dict(loss_kind=loss, s_pos=s_pos, s_neg=s_neg, e_pos=e_pos, e_neg=e_neg, lr=float(lr))
    if loss == 'bpr':
        x = s_neg - s_pos.unsqueeze(1)
        sig = torch.sigmoid(x)
        dneg = sig / (n * Q)
        dpos = -dneg.sum(1)
        ref.update(x=x, sig=sig, loss=torch.nn.functional.softplus(x).mean(), terms=torch.nn.functional.softplus(x) / (n * Q))
    else:
        lq_neg = logq[neg].double() if logq is not None else torch.zeros_like(s_neg)
        lq_pos = logq[pos].double() if logq is not None else torch.zeros_like(s_pos)
        z_neg, z_pos = s_neg - lq_neg, s_pos - lq_pos
        lse = torch.logsumexp(torch.cat([z_pos.unsqueeze(1), z_neg], 1), 1)
        dneg = torch.exp(z_neg - lse.unsqueeze(1)) / Q
        dpos = (torch.exp(z_pos - lse) - 1.0) / Q
        ref.update(z_neg=z_neg, z_pos=z_pos, lse=lse, lq_neg=lq_neg, lq_pos=lq_pos, loss=(lse - z_pos).mean())
    qg = dpos.unsqueeze(1) * wp
    for lo in range(0, Q, 16):
        qg[lo:lo + 16] += (dneg[lo:lo + 16].unsqueeze(-1) * W[neg[lo:lo + 16]].double()).sum(1)
    grad = torch.zeros(N, d, dtype=torch.float64, device=W.device)
    grad.index_add_(0, pos, dpos.unsqueeze(1) * q64)
    for lo in range(0, Q, 16):
        grad.index_add_(0, neg[lo:lo + 16].reshape(-1), (dneg[lo:lo + 16].unsqueeze(-1) * q64[lo:lo + 16].unsqueeze(1)).reshape(-1, d))
    if step['pad']:
        grad[0] = 0
    ref.update(dneg=dneg, dpos=dpos, qgrad=qg, grad=grad, W_after=W.double() - float(lr) * grad, owners=[])
    for ow in step['owners']:
        eq, ej = ow['eq'], ow['ej']
        de = dneg[eq, ej]
        r = dict(d=de, dsum=torch.zeros(Q, dtype=torch.float64, device=W.device).index_add_(0, eq, de),
                 K=torch.bincount(eq, minlength=Q))
        if loss == 'bpr':
            r['loss'] = ref['terms'][eq, ej].sum()
        else:
            z = ref['z_neg'][eq, ej]
            m = torch.full((Q,), -float('inf'), dtype=torch.float64, device=W.device).scatter_reduce(0, eq, z, 'amax')
            e = torch.exp(z - m[eq])
            r.update(z=z, run_max=m, run_sum=torch.zeros_like(m).index_add_(0, eq, e),
                     run_acc=torch.zeros(Q, d, dtype=torch.float64, device=W.device).index_add_(0, eq, e.unsqueeze(1) * ow['table'][ow['rows']].double()))
        ref['owners'].append(r)
    return ref


def reduce_lse(run_max, run_sum, z_pos):
    """The (max, rescaled sum) reduction over the owners as ShardedItemTable.ssm_step_on_owners performs it; run_max / run_sum
    [G, Q] in any float type -> lse [Q]."""
    m = torch.maximum(run_max.amax(0), z_pos)
    s = (run_sum * torch.exp(run_max - m)).sum(0)
    return m + torch.log(s + torch.exp(z_pos - m))


def sharded_bookkeeping(step, ref):
    """The referee's own per-owner partials pushed through the owner protocol in float64 -> dict(dpos, lse, qgrad, grad): must
    equal the unsharded step up to float64 rounding."""
    Q, d, N, G, lay = step['Q'], step['d'], step['N'], step['G'], step['layout']
    dev = step['W'].device
    bpr = ref['loss_kind'] == 'bpr'
    out = {}
    if bpr:
        dpos = -torch.stack([r['dsum'] for r in ref['owners']]).sum(0)
    else:
        out['lse'] = reduce_lse(torch.stack([r['run_max'] for r in ref['owners']]), torch.stack([r['run_sum'] for r in ref['owners']]),
                                ref['z_pos'])
        dpos = (torch.exp(ref['z_pos'] - out['lse']) - 1.0) / Q
    qg = torch.zeros(Q, d, dtype=torch.float64, device=dev)
    blocks = []
    for ow, r in zip(step['owners'], ref['owners']):
        t64, q64 = ow['table'].double(), step['q_all'].double()
        own = ow['pos_rows'] >= 0
        prow = ow['pos_rows'].clamp(min=0)
        if bpr:
            qg.index_add_(0, ow['eq'], r['d'].unsqueeze(1) * t64[ow['rows']])
            de = r['d']
        else:
            live = r['run_max'] > -float('inf')
            c = torch.where(live, torch.exp(r['run_max'] - out['lse']) / Q, torch.zeros_like(out['lse']))
            qg += c.unsqueeze(1) * r['run_acc']
            de = torch.exp(r['z'] - out['lse'][ow['eq']]) / Q
        qg += torch.where(own, dpos, torch.zeros_like(dpos)).unsqueeze(1) * t64[prow]
        blk = torch.zeros(ow['n_rows'], d, dtype=torch.float64, device=dev)
        blk.index_add_(0, ow['rows'], de.unsqueeze(1) * q64[ow['eq']])
        blk.index_add_(0, prow[own], (dpos.unsqueeze(1) * q64)[own])
        if ow['pad_row'] >= 0:
            blk[ow['pad_row']] = 0
        blocks.append(blk)
    full = torch.zeros(N, d, dtype=torch.float64, device=dev)
    for o, blk in enumerate(blocks):
        take(full, o, N, G, lay).copy_(blk)
    out.update(dpos=dpos, qgrad=qg, grad=full)
    return out


# -------------------------------------------------------------------------------------------------------------------- allowances
def _units(got, want):
    return float(((got.double() - want).abs() / (U32 * want.abs().clamp_min(1e-300))).max())


def allowances(device, Q, n):
    """Twice the measured worst error, in units of u x the result, of torch's fp32 sigmoid (scaled as the step scales it:
    sgd_referee.torch_sigmoid_allowance), exp and log(1 + t) on ``device`` against float64 at the same fp32 arguments -> dict(sig,
    exp, log, measured=(sig, exp, log))."""
    import sgd_referee as sg
    a_sig, m_sig = sg.torch_sigmoid_allowance(device, Q, n)
    g = torch.Generator(device=device).manual_seed(0)
    k = 1 << 18
    x = torch.cat([torch.linspace(-30, 0, k, device=device)] + [-(torch.randn(k, device=device, generator=g) * w).abs() for w in (0.1, 1.0, 4.0)])
    m_exp = _units(torch.exp(x), torch.exp(x.double()))
    t = torch.exp(x)
    m_log = _units(torch.log(1.0 + t), torch.log((1.0 + t).double()))       # (the rounded 1 + t is the fp32 argument)
    return dict(sig=a_sig, exp=2.0 * m_exp, log=2.0 * m_log, measured=(m_sig, m_exp, m_log))


ZERO_ALLOW = dict(sig=0.0, exp=0.0, log=0.0)


# ------------------------------------------------------------------------------------------------------------------------- judging
def _ratio(got, want, tol):
    err = (got.double() - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
    return float(r.max()) if r.numel() else 0.0


def _rows_stage_a(step, ow, d_slot, dpos32, scale, target0):
    """Stage A of one owner's rows from fp32 coefficients: (want [n_rows, d], tol [n_rows, d]) for target0 + scale * g."""
    Q = step['Q']
    dev = step['W'].device
    own = ow['pos_rows'] >= 0
    ids = torch.cat([ow['rows'], ow['pos_rows'][own]]).view(-1, 1)
    coef = torch.cat([d_slot.double(), dpos32.double()[own]]).view(-1, 1)
    qidx = torch.cat([ow['eq'], torch.arange(Q, device=dev)[own]])
    gr = ar.row_gradients(step['q_all'], ids, coef, query_index=qidx, pad_row=ow['pad_row'] if ow['pad_row'] >= 0 else -9)
    want = target0.double().clone()
    want[gr['rows']] += float(scale) * gr['g']
    tol = 2 * U32 * want.abs()
    tol[gr['rows']] += abs(float(scale)) * (gr['K'].double().unsqueeze(1) + 2.0) * U32 * gr['A']
    return want, tol, gr


def bpr_tolerances(step, ref, allow, exp_argument_term=True):
    """Stage B of BPR per owner -> list of dict(tol_d [E_o], tol_dsum [Q], tol_loss)."""
    Q, n = step['Q'], step['n']
    out = []
    for ow, r in zip(step['owners'], ref['owners']):
        eq, ej = ow['eq'], ow['ej']
        x, sig = ref['x'][eq, ej], ref['sig'][eq, ej]
        ex = ref['e_neg'][eq, ej] + ref['e_pos'][eq]
        arg = ex + (2 * U32 * x.abs() if exp_argument_term else 0.0)
        tol_d = r['d'] * ((1.0 - sig) * arg + allow['sig'] * U32)
        tol_dsum = torch.zeros(Q, dtype=torch.float64, device=x.device).index_add_(0, eq, tol_d)
        tol_dsum += (r['K'].double() - 1).clamp_min(0) * U32 * r['dsum']
        sp = torch.nn.functional.softplus(x)
        tol_loss = float(((sig * arg + (max(allow['exp'], allow['log']) + 4.0) * U32 * sp) / (n * Q)).sum() + eq.numel() * U32 * r['loss'])
        out.append(dict(tol_d=tol_d, tol_dsum=tol_dsum, tol_loss=tol_loss))
    return out


def judge_bpr(step, ref, out, allow, inplace, exp_argument_term=True):
    """``out``: what an implementation left -- pos_score [Q]; per owner d_slots [slots + Q], dsum_part [Q], loss_part, qgrad [Q, d],
    target (the gradient block, or the table after the in-place step).  -> dict stage -> worst |error| / bound."""
    Q, G, d = step['Q'], step['G'], step['d']
    lr = ref['lr']
    res = {'pos_score': _ratio(out['pos_score'], ref['s_pos'], ref['e_pos'] + 1e-300)}
    tols = bpr_tolerances(step, ref, allow, exp_argument_term)
    dsum_all = torch.stack([o['dsum_part'] for o in out['owners']]).sum(0)
    res['B.d_slots'] = res['B.dsum_part'] = res['A.rows'] = res['E.rows'] = 0.0
    loss_got, loss_tol = 0.0, 0.0
    qg_got = torch.zeros(Q, d, dtype=torch.float64, device=step['W'].device)
    qg_want, qg_tol = torch.zeros_like(qg_got), torch.zeros_like(qg_got)
    e2e_want, e2e_tol = torch.zeros_like(qg_got), torch.zeros_like(qg_got)
    empty_exact = True
    for o, (ow, r, t, oo) in enumerate(zip(step['owners'], ref['owners'], tols, out['owners'])):
        d32 = oo['d_slots'][ow['slot']]
        res['B.d_slots'] = max(res['B.d_slots'], _ratio(d32, r['d'], t['tol_d']))
        res['B.dsum_part'] = max(res['B.dsum_part'], _ratio(oo['dsum_part'], r['dsum'], t['tol_dsum']))
        empty_exact &= bool((oo['dsum_part'][r['K'] == 0] == 0).all())
        loss_got += float(oo['loss_part'].double())
        loss_tol += t['tol_loss']
        own = ow['pos_rows'] >= 0
        dpos32 = torch.where(own, -dsum_all, torch.zeros_like(dsum_all))
        # Stage A of the query gradients: this owner's share from ITS fp32 coefficients
        t64 = ow['table'].double()
        prow = ow['pos_rows'].clamp(min=0)
        terms = d32.double().unsqueeze(1) * t64[ow['rows']]
        pterm = dpos32.double().unsqueeze(1) * t64[prow]
        want = torch.zeros_like(qg_got).index_add_(0, ow['eq'], terms) + pterm
        A = torch.zeros_like(qg_got).index_add_(0, ow['eq'], terms.abs()) + pterm.abs()
        qg_got += oo['qgrad'].double()
        qg_want += want
        qg_tol += (r['K'].double() + own.double() + 3.0).unsqueeze(1) * U32 * A
        # Stage B carried through: the float64 coefficients' share and what the coefficients' bounds allow
        tol_dpos = torch.stack([x['tol_dsum'] for x in tols]).sum(0) + (G - 1) * U32 * ref['dpos'].abs()
        e2e_want += torch.zeros_like(qg_got).index_add_(0, ow['eq'], r['d'].unsqueeze(1) * t64[ow['rows']]) + \
            torch.where(own, ref['dpos'], torch.zeros_like(ref['dpos'])).unsqueeze(1) * t64[prow]
        e2e_tol += torch.zeros_like(qg_got).index_add_(0, ow['eq'], t['tol_d'].unsqueeze(1) * t64[ow['rows']].abs()) + \
            torch.where(own, tol_dpos, torch.zeros_like(tol_dpos)).unsqueeze(1) * t64[prow].abs()
        # rows: Stage A from the fp32 coefficients, end to end against the float64 step
        scale = -lr if inplace else 1.0
        t0 = ow['table'] if inplace else torch.zeros_like(ow['table'])
        want_a, tol_a, gr = _rows_stage_a(step, ow, d32, dpos32, scale, t0)
        res['A.rows'] = max(res['A.rows'], _ratio(oo['target'], want_a, tol_a))
        slack = _rows_stage_a(step, ow, t['tol_d'], tol_dpos, 1.0, torch.zeros_like(ow['table']))[2]
        want_e = take(ref['W_after'] if inplace else ref['grad'], o, step['N'], G, step['layout'])
        tol_e = tol_a.clone()
        tol_e[slack['rows']] += abs(scale) * slack['A']
        res['E.rows'] = max(res['E.rows'], _ratio(oo['target'], want_e, tol_e))
    res['B.loss'] = abs(loss_got - float(ref['loss'])) / loss_tol
    res['A.qgrad'] = _ratio(qg_got, qg_want, qg_tol)
    res['E.qgrad'] = _ratio(qg_got, ref['qgrad'], qg_tol + e2e_tol)
    assert torch.allclose(e2e_want, ref['qgrad'], rtol=1e-12, atol=1e-18)
    res['empty_dsum_exact'] = 0.0 if empty_exact else float('inf')
    return res


def ssm_tolerances(step, ref, allow):
    """Stage B of SampledSoftmax per owner and for the reduced quantities."""
    Q, G = step['Q'], step['G']
    per = []
    dev = step['W'].device
    tol_lse = torch.zeros(Q, dtype=torch.float64, device=dev)
    z_all = torch.cat([ref['z_pos'].unsqueeze(1), ref['z_neg']], 1)
    rng_z = z_all.amax(1) - z_all.amin(1)
    K_all = float(step['n'] + 1)
    for ow, r in zip(step['owners'], ref['owners']):
        eq, ej = ow['eq'], ow['ej']
        tol_z = ref['e_neg'][eq, ej] + 2 * U32 * r['z'].abs() + U32 * ref['lq_neg'][eq, ej].abs()
        K = r['K'].double()
        rel = (2 * K + 20) * U32 + (K + 9) * allow['exp'] * U32 + 4 * U32 * rng_z
        per.append(dict(tol_z=tol_z, rel=rel))
        p = torch.exp(r['z'] - ref['lse'][eq])
        tol_lse.index_add_(0, eq, p * (tol_z + rel[eq]))
    tol_zpos = ref['e_pos'] + 2 * U32 * ref['z_pos'].abs() + U32 * ref['lq_pos'].abs()
    # the restated reduction: G + 1 exps, a log, a dozen fp32 operations on values of size <= |lse| + 1
    tol_lse += torch.exp(ref['z_pos'] - ref['lse']) * tol_zpos + (G + 2) * (max(allow['exp'], allow['log']) + 4.0) * U32 * (1.0 + ref['lse'].abs())
    tol_dpos = torch.exp(ref['z_pos'] - ref['lse']) / Q * (tol_zpos + tol_lse + (allow['exp'] + 2 * (ref['z_pos'] - ref['lse']).abs()) * U32) \
        + 2 * U32 * ref['dpos'].abs()
    for ow, r, t in zip(step['owners'], ref['owners'], per):
        eq = ow['eq']
        arg = (r['z'] - ref['lse'][eq]).abs()
        t['tol_d'] = r['d'] * (t['tol_z'] + tol_lse[eq] + 2 * U32 * arg + (allow['exp'] + 1.0) * U32)
    return per, tol_zpos, tol_lse, tol_dpos, K_all


def judge_ssm(step, ref, out, allow, inplace):
    """``out``: z_pos [Q] (fp32, as handed to the finish), lse [Q]; per owner z_slots [slots] (phase 1), run_max, run_sum, run_acc,
    d_slots (phase 2 of the gradient-block form: d of every live slot; may be None), qgrad [Q, d], target."""
    Q, G, d = step['Q'], step['G'], step['d']
    lr = ref['lr']
    dev = step['W'].device
    per, tol_zpos, tol_lse, tol_dpos, _ = ssm_tolerances(step, ref, allow)
    res = {'z_pos': _ratio(out['z_pos'], ref['z_pos'], tol_zpos), 'B.lse': _ratio(out['lse'], ref['lse'], tol_lse)}
    for k in ('B.z', 'B.run_sum', 'B.run_acc', 'B.d_slots', 'A.rows', 'E.rows'):
        res[k] = 0.0
    exact = True
    finite = bool(torch.isfinite(out['lse']).all())
    qg_got = torch.zeros(Q, d, dtype=torch.float64, device=dev)
    qg_tol = torch.zeros_like(qg_got)
    dpos32 = (torch.exp(out['z_pos'].double() - out['lse'].double()) - 1.0) / Q      # what the finish derives, in float64
    for o, (ow, r, t, oo) in enumerate(zip(step['owners'], ref['owners'], per, out['owners'])):
        eq = ow['eq']
        z32 = oo['z_slots'][ow['slot']]
        res['B.z'] = max(res['B.z'], _ratio(z32, r['z'], t['tol_z']))
        has = r['K'] > 0
        exact &= bool((oo['run_max'][~has] == -float('inf')).all()) and bool((oo['run_sum'][~has] == 0).all())
        own_max = torch.full((Q,), -float('inf'), dtype=torch.float32, device=dev).scatter_reduce(0, eq, z32, 'amax')
        exact &= bool(torch.equal(oo['run_max'], own_max))
        # against the kernel's OWN maximum: sum exp(z64 - run_max32) [row]
        m32 = oo['run_max'].double()
        e = torch.exp(r['z'] - m32[eq])
        t64 = ow['table'].double()
        want_s = torch.zeros(Q, dtype=torch.float64, device=dev).index_add_(0, eq, e)
        tol_s = torch.zeros_like(want_s).index_add_(0, eq, e * (t['tol_z'] + t['rel'][eq]))
        terms = e.unsqueeze(1) * t64[ow['rows']]
        want_a = torch.zeros(Q, d, dtype=torch.float64, device=dev).index_add_(0, eq, terms)
        tol_acc = torch.zeros_like(want_a).index_add_(0, eq, terms.abs() * (t['tol_z'] + t['rel'][eq]).unsqueeze(1))
        res['B.run_sum'] = max(res['B.run_sum'], _ratio(oo['run_sum'][has], want_s[has], tol_s[has]))
        res['B.run_acc'] = max(res['B.run_acc'], _ratio(oo['run_acc'][has], want_a[has], tol_acc[has]))
        finite &= all(bool(torch.isfinite(x).all()) for x in (oo['run_sum'], oo['run_acc'], oo['qgrad'], oo['target']))
        own = ow['pos_rows'] >= 0
        prow = ow['pos_rows'].clamp(min=0)
        qg_got += oo['qgrad'].double()
        dterm = r['d'].unsqueeze(1) * t64[ow['rows']]
        qg_tol += torch.zeros_like(qg_got).index_add_(0, eq, t['tol_d'].unsqueeze(1) * t64[ow['rows']].abs() + dterm.abs() * t['rel'][eq].unsqueeze(1))
        qg_tol += (torch.where(own, tol_dpos, torch.zeros_like(tol_dpos)) + 3 * U32 * ref['dpos'].abs() * own).unsqueeze(1) * t64[prow].abs()
        scale = -lr if inplace else 1.0
        t0 = ow['table'] if inplace else torch.zeros_like(ow['table'])
        if oo.get('d_slots') is not None:
            d32 = oo['d_slots'][ow['slot']]
            res['B.d_slots'] = max(res['B.d_slots'], _ratio(d32, r['d'], t['tol_d']))
            want_r, tol_r, _ = _rows_stage_a(step, ow, d32, torch.where(own, dpos32, torch.zeros_like(dpos32)), scale, t0)
            # (dpos32 is the finish's own value up to its exp, its 1 - p and its scaling)
            dp_slack = _rows_stage_a(step, ow, torch.zeros_like(t['tol_d']), (allow['exp'] + 4.0) * U32 * dpos32.abs() + U32 / Q, 1.0,
                                     torch.zeros_like(ow['table']))[2]
            tol_r[dp_slack['rows']] += abs(scale) * dp_slack['A']
            res['A.rows'] = max(res['A.rows'], _ratio(oo['target'], want_r, tol_r))
        _, tol_a, gr = _rows_stage_a(step, ow, r['d'], torch.where(own, ref['dpos'], torch.zeros_like(ref['dpos'])), scale, t0)
        slack = _rows_stage_a(step, ow, t['tol_d'], tol_dpos, 1.0, torch.zeros_like(ow['table']))[2]
        tol_a[slack['rows']] += abs(scale) * slack['A']
        want_e = take(ref['W_after'] if inplace else ref['grad'], o, step['N'], G, step['layout'])
        res['E.rows'] = max(res['E.rows'], _ratio(oo['target'], want_e, tol_a))
    res['E.qgrad'] = _ratio(qg_got, ref['qgrad'], qg_tol + 4 * U32 * ref['qgrad'].abs())
    res['exact_runs'] = 0.0 if exact else float('inf')
    res['finite'] = 0.0 if finite else float('inf')
    return res


def judge_gated(step, out):
    """A gated step: every table and every owner's qgrad bit-unchanged, step_dropped == the sum of the header words."""
    bad = 0
    for ow, oo in zip(step['owners'], out['owners']):
        want = int(ow['keys'].view(-1, step['stride'])[:, 1].sum())
        bad += int(not torch.equal(oo['target'], ow['table'])) + int(bool((oo['qgrad'] != 0).any())) + int(int(oo['step_dropped']) != want)
    return bad


# ------------------------------------------------------------------------------------------------------------- the fp32 emulation
def emulate(step, loss, lr, inplace, mistake=None, use_logq=True):
    """The owner protocol in torch fp32, owner by owner, READ FROM THE SEGMENTS as the kernels read them (live counts, dead keys,
    header word 1), the reductions in between; ``mistake``: one of MISTAKES.  -> ``out`` as judge_bpr / judge_ssm / judge_gated take it."""
    assert mistake is None or mistake in MISTAKES
    f32 = torch.float32
    Q, G, B, n, d, stride, cap = step['Q'], step['G'], step['B'], step['n'], step['d'], step['stride'], step['cap']
    dev = step['W'].device
    q_all = step['q_all']
    mean_den = B if mistake == 'mean_over_local_batch' else Q
    binv, bw = torch.tensor(1.0 / mean_den, dtype=f32), torch.tensor(1.0 / n, dtype=f32)
    parsed = []
    for ow in step['owners']:
        k = ow['keys'].view(-1, stride)
        within = torch.arange(stride, device=dev).unsqueeze(0)
        live = (within >= HDR) & ((within - HDR < k[:, :1]) | (mistake == 'slack_is_live'))
        kq, kr = (k >> 32) & 0x7fffffff, k & 0xffffffff
        ok = (live & (kq < Q) & (kr < ow['n_rows'])).reshape(-1)
        slot = ok.nonzero().view(-1)
        eq, er = kq.reshape(-1)[slot], kr.reshape(-1)[slot]
        if mistake == 'ragged_tail_dropped':          # the last len % 64 elements of every run never reach a tile
            order = torch.argsort(eq, stable=True)
            sq = eq[order]
            first = torch.ones_like(sq, dtype=torch.bool)
            first[1:] = sq[1:] != sq[:-1]
            start = torch.cummax(torch.where(first, torch.arange(sq.numel(), device=dev), torch.zeros_like(sq)), 0)[0]
            rank = torch.arange(sq.numel(), device=dev) - start
            length = torch.bincount(sq, minlength=Q)[sq]
            keep = order[rank < (length // 64) * 64].sort()[0]
            slot, eq, er = slot[keep], eq[keep], er[keep]
        dropped = int(k[:, 1].sum())
        gate = 1.0 if (dropped == 0 or mistake == 'gate_ignored') else 0.0
        dot = (q_all[eq] * ow['table'][er]).sum(-1)
        parsed.append(dict(slot=slot, eq=eq, er=er, dot=dot, gate=gate, dropped=dropped))
    own_mask = [ow['pos_rows'] >= 0 for ow in step['owners']]
    pos_score = torch.stack([torch.where(m, (q_all * ow['table'][ow['pos_rows'].clamp(min=0)]).sum(-1), torch.zeros(Q, device=dev))
                             for m, ow in zip(own_mask, step['owners'])]).sum(0)
    out = dict(pos_score=pos_score, owners=[])
    if loss == 'bpr':
        for p in parsed:
            x = p['dot'] - pos_score[p['eq']]
            p['d'] = torch.sigmoid(x) * bw * binv
            p['dsum'] = torch.zeros(Q, dtype=f32, device=dev).index_add_(0, p['eq'], p['d'])
            p['loss'] = (torch.nn.functional.softplus(x) * bw).sum() * binv
        dsum_all = torch.stack([p['dsum'] for p in parsed]).sum(0)
        dpos = [-(p['dsum'] if mistake == 'local_dsum' else dsum_all) for p in parsed]
    else:
        lq = step['logq'] is not None and use_logq
        z_pos = pos_score - (step['logq'][step['pos']] if lq else 0.0)
        for p, ow in zip(parsed, step['owners']):
            p['z'] = p['dot'] - (ow['logq_rows'][p['er']] if lq else 0.0)
            p['run_max'] = torch.full((Q,), -float('inf'), dtype=f32, device=dev).scatter_reduce(0, p['eq'], p['z'], 'amax')
            e = torch.exp(p['z'] - p['run_max'][p['eq']])
            p['run_sum'] = torch.zeros(Q, dtype=f32, device=dev).index_add_(0, p['eq'], e)
            p['run_acc'] = torch.zeros(Q, d, dtype=f32, device=dev).index_add_(0, p['eq'], e.unsqueeze(1) * ow['table'][p['er']])
        rm, rs = torch.stack([p['run_max'] for p in parsed]), torch.stack([p['run_sum'] for p in parsed])
        if mistake == 'merge_without_rescale':
            m = torch.maximum(rm.amax(0), z_pos)
            lse = m + torch.log(rs.sum(0) + torch.exp(z_pos - m))
        else:
            lse = reduce_lse(rm, rs, z_pos)
        for p in parsed:
            p['d'] = torch.exp(p['z'] - lse[p['eq']]) * binv
        dpos = [-(1.0 - torch.exp(z_pos - lse)) * binv] * G
        out.update(z_pos=z_pos, lse=lse)
    for o, (p, ow) in enumerate(zip(parsed, step['owners'])):
        gate = p['gate']
        own = own_mask[o]
        if mistake == 'pos_by_non_owner':
            own = own_mask[(o - 1) % G]                   # the neighbour's positives instead of its own
            prow = step['owners'][(o - 1) % G]['pos_rows'].clamp(min=0, max=ow['n_rows'] - 1)
        else:
            prow = ow['pos_rows'].clamp(min=0)
        dp = torch.where(own, dpos[o], torch.zeros_like(dpos[o]))
        table = ow['table']
        if loss == 'bpr':
            qg = torch.zeros(Q, d, dtype=f32, device=dev).index_add_(0, p['eq'], p['d'].unsqueeze(1) * table[p['er']])
        else:
            live = p['run_max'] > -float('inf')
            c = torch.where(live, torch.ones_like(lse) if mistake == 'acc_without_rescale' else torch.exp(p['run_max'] - lse),
                            torch.zeros_like(lse)) * binv
            qg = c.unsqueeze(1) * p['run_acc']
        qg = gate * (qg + dp.unsqueeze(1) * table[prow])
        rows = torch.cat([p['er'], prow[own]])
        coef = torch.cat([p['d'], dp[own]])
        qi = torch.cat([p['eq'], torch.arange(Q, device=dev)[own]])
        if ow['pad_row'] >= 0 and mistake != 'padding_row_updated':
            keep = rows != ow['pad_row']
            rows, coef, qi = rows[keep], coef[keep], qi[keep]
        g = torch.zeros(ow['n_rows'], d, dtype=f32, device=dev).index_add_(0, rows, coef.unsqueeze(1) * q_all[qi])
        scale = torch.tensor((-float(lr) if inplace else 1.0) * gate, dtype=f32)
        target = (table if inplace else torch.zeros_like(table)) + scale * g
        if mistake == 'solo_twice' and inplace:
            solo = torch.bincount(rows, minlength=ow['n_rows']) == 1
            target[solo] = target[solo] + scale * g[solo]
        d_slots = torch.zeros(step['slots'] + Q, dtype=f32, device=dev)
        d_slots[p['slot']] = p['d']
        oo = dict(d_slots=d_slots, qgrad=qg, target=target, step_dropped=p['dropped'])
        if loss == 'bpr':
            oo.update(dsum_part=p['dsum'], loss_part=p['loss'])
        else:
            z_slots = torch.zeros(step['slots'], dtype=f32, device=dev)
            z_slots[p['slot']] = p['z']
            oo.update(z_slots=z_slots, run_max=p['run_max'], run_sum=p['run_sum'], run_acc=p['run_acc'])
        out['owners'].append(oo)
    return out


def worst(res):
    return max(res.values())
