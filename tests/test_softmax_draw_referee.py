"""CPU: the float64 referee of exact softmax sampling (tests/softmax_draw_referee.py) -- an fp32 emulation of the three steps stays
inside half of every tolerance, eight seeded mistakes each leave a tolerance or trip an exact condition, and the reference's op
sequence (baseretriever.py:313-328, restated with CPU torch) gives the referee's log-probabilities."""
import pytest
import torch

import softmax_draw_referee as R

G = 64
COUNTS = ('outside', 'zero_weight', 'block', 'item', 'logp')


def case(mode, d, t, n_cols, M=6, n=40, seed=0, hist_len=12):
    """A catalog with a few heavy items, a history that holds some of them twice, 0-padding, and one block wholly inside it."""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(n_cols + 1, d, generator=g) * 0.4
    W[0] = 0
    Q = torch.randn(M, d, generator=g) * 0.6
    heavy = torch.randint(1, n_cols + 1, (M, 3), generator=g)
    for b in range(M):
        W[heavy[b]] += Q[b] * (1.5 if mode != R.COS else 0.2)
    hist = torch.randint(1, n_cols + 1, (M, hist_len), generator=g)
    hist[:, :3] = heavy
    hist[:, 3:5] = heavy[:, :2]                                    # duplicates of heavy ids
    hist[:, -2:] = 0                                               # padding
    if n_cols < 4 * hist_len:                                      # a tiny catalog: one heavy id, twice, and padding
        hist = torch.cat([heavy[:, :1], heavy[:, :1], torch.zeros(M, 2, dtype=torch.long)], dim=1)
    if n_cols >= 2 * G:
        hist = torch.cat([hist, torch.arange(G + 1, 2 * G + 1).expand(M, G)], dim=1)      # block 1 wholly in the history
    pos = torch.randint(0, n_cols + 1, (M, 2), generator=g)
    u = torch.rand(M, n, 2, generator=g)
    return W, Q, hist, pos, u


def violations(res):
    return {k: res[k] for k in COUNTS if res[k]}


@pytest.mark.parametrize('mode,d,t,n_cols', [(R.IP, 32, 1.0, 5), (R.IP, 64, 0.5, G - 1), (R.COS, 48, 4.0, G), (R.EUC, 32, 1.0, 3 * G + 5),
                                              (R.IP, 128, 4.0, 3 * G + 5), (R.COS, 64, 0.5, 3 * G + 5), (R.EUC, 64, 4.0, 1000)])
@pytest.mark.parametrize('with_hist', [False, True])
def test_fp32_emulation_stays_inside_half_of_every_tolerance(mode, d, t, n_cols, with_hist):
    W, Q, hist, pos, u = case(mode, d, t, n_cols)
    hist = hist if with_hist else None
    T = R.tables64(W, Q, t, mode, G, hist)
    u = torch.cat([u, R.edge_uniforms(T, 24, torch.Generator().manual_seed(5))], dim=1)
    ids, logp, pos_logp, lse = R.emulate(W, Q, t, mode, G, u, hist=hist, pos=pos)
    res = R.judge_draws(T, ids, u, logp, scale=0.5)
    assert not violations(res), res
    assert R.judge_logp(T, pos, pos_logp, scale=0.5)[0] == 0
    assert R.judge_lse(T, lse, scale=0.5)[0] == 0
    if with_hist:
        assert not (ids.unsqueeze(2) == hist.unsqueeze(1)).any()
        if n_cols >= 2 * G:
            assert float(T['mass'][:, 1].abs().max()) == 0.0


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_seeded_mistakes_are_caught(mistake):
    mode = R.COS if mistake == 'ip_lse_with_cosine' else R.IP
    t = 4.0 if mistake == 'temperature_on_lse_only' else 1.0
    W, Q, hist, pos, u = case(mode, 64, t, 3 * G + 5, n=200, seed=1)
    T = R.tables64(W, Q, t, mode, G, hist)
    ids, logp, _, _ = R.emulate(W, Q, t, mode, G, u, hist=hist)
    good = R.judge_draws(T, ids, u, logp)
    assert not violations(good), good
    ids, logp, _, _ = R.emulate(W, Q, t, mode, G, u, hist=hist, mistake=mistake)
    bad = R.judge_draws(T, ids, u, logp)
    assert violations(bad), (mistake, bad)


def test_own_block_rule():
    cum = torch.tensor([[0.25, 0.25, 0.75, 1.0, 1.0]])
    u1 = torch.tensor([[0.0, 0.2499, 0.25, 0.5, 0.75, 0.99, 1.0]])
    assert R.own_block(cum, u1).tolist() == [[0, 0, 2, 2, 3, 3, 3]]


@pytest.mark.parametrize('mode', [R.IP, R.COS, R.EUC])
@pytest.mark.parametrize('excluding_hist', [False, True])
def test_reference_op_sequence_gives_the_referees_log_probabilities(mode, excluding_hist):
    """baseretriever.py:313-328 with CPU torch: softmax, pad, gather, mask_with_hist (a scatter of zeros), multinomial, log of the gather."""
    t = 0.5
    W, Q, hist, pos, _ = case(mode, 32, t, 3 * G + 5, seed=2)
    item_vector, q = W[1:], Q
    if mode == R.IP:
        score = q @ item_vector.t()
    elif mode == R.COS:
        score = (q / q.norm(dim=1, keepdim=True)) @ (item_vector / item_vector.norm(dim=1, keepdim=True)).t()
    else:
        score = -((item_vector ** 2).sum(1) + (q ** 2).sum(1, keepdim=True) - 2 * q @ item_vector.t())
    all_prob = torch.nn.functional.pad(torch.softmax(score / t, dim=-1), pad=(1, 0))
    log_pos_prob = torch.log(torch.gather(all_prob, dim=-1, index=pos))
    sampling_prob = all_prob.scatter(-1, hist, 0.0) if excluding_hist else all_prob
    torch.manual_seed(0)
    neg_id = torch.multinomial(sampling_prob, 50, replacement=True)
    log_neg_prob = torch.log(torch.gather(sampling_prob, dim=-1, index=neg_id))
    T = R.tables64(W, Q, t, mode, G, hist if excluding_hist else None)
    assert R.judge_logp(T, neg_id, log_neg_prob)[0] == 0
    assert R.judge_logp(T, pos, log_pos_prob)[0] == 0
    assert int((T['w'].gather(1, neg_id) <= 0).sum()) == 0
    # and the masked row the reference draws from is the referee's w
    assert float((sampling_prob.double() - T['w']).abs().max()) <= float((T['eps'].max() + T['eps_lse'].max()) * 2)
