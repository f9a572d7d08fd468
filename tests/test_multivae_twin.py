"""CPU: MultiDAEQueryEncoder / MultiVAEQueryEncoder and UserDataset against tests/golden/multivae.npz, a recording of the
reference's own classes (tools/make_golden_multivae.py).  Encoders: 1e-4 on outputs, 3e-4 on gradients (the tolerances of
tests/test_caser_twin.py); the dataset: exactly."""
import numpy as np
import pytest
import torch

from recstudio_amd import MultiDAEQueryEncoder, MultiVAEQueryEncoder, UserDataset

from test_dataset_golden import make, seed_everything

ENC_DIMS, DEC_DIMS = [6, 4], [4, 6]
ENCODERS = {'dae': (MultiDAEQueryEncoder, 'relu', ('item_embedding', 'encoder_decoder')),
            'vae': (MultiVAEQueryEncoder, 'tanh', ('item_embedding', 'encoders', 'decoders'))}


def build(g, name, fused_bag=False):
    cls, act, _ = ENCODERS[name]
    n_items, d = g[f'{name}.sd.item_embedding.weight'].shape
    enc = cls('item_id', n_items, d, 0.0, ENC_DIMS, DEC_DIMS, act, fused_bag=fused_bag)
    sd = {k[len(name) + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f'{name}.sd.')}
    enc.load_state_dict(sd, strict=True)
    return enc, sd


@pytest.mark.parametrize('name', sorted(ENCODERS))
def test_state_dict_keys_are_the_reference_s(golden, name):
    g = golden('multivae')
    enc, sd = build(g, name)
    assert list(enc.state_dict()) == list(sd)
    assert {k.split('.')[0] for k in sd} == set(ENCODERS[name][2])
    assert enc.item_embedding.padding_idx == 0


@pytest.mark.parametrize('name', sorted(ENCODERS))
def test_encoder_matches_the_recording(golden, name):
    g = golden('multivae')
    enc, _ = build(g, name)
    batch = {'in_item_id': torch.from_numpy(g['in_item_id'])}
    enc.eval()
    with torch.no_grad():
        np.testing.assert_allclose(enc(batch).numpy(), g[f'{name}.eval'], rtol=1e-4, atol=1e-6)
    enc.train()
    torch.manual_seed(77)
    out = enc(batch)
    np.testing.assert_allclose(out.detach().numpy(), g[f'{name}.train'], rtol=1e-4, atol=1e-6)
    params = dict(enc.named_parameters())
    grads = torch.autograd.grad((out * torch.from_numpy(g['g'])).sum(), list(params.values()))
    for k, gr in zip(params, grads):
        np.testing.assert_allclose(gr.numpy(), g[f'{name}.grad.{k}'], rtol=3e-4, atol=1e-6, err_msg=k)
    if name == 'vae':
        np.testing.assert_allclose(float(enc.kl_loss), float(g['vae.kl']), rtol=1e-4)
        enc.eval()
        with torch.no_grad():
            a, b = enc(batch), enc(batch)
        assert torch.equal(a, b)                          # eval: z = mu, no draw


def test_user_dataset_matches_the_recording(golden):
    g, data = golden('multivae'), golden('data_ml100k')
    seed_everything(2022)
    ds = make(UserDataset, data)
    splits = ds.build(split_ratio=[0.8, 0.1, 0.1], shuffle=True, split_mode='user_entry')
    assert [len(s) for s in splits] == g['u.counts'].tolist()
    for name, split in zip(('trn', 'val', 'tst'), splits):
        assert np.array_equal(split.data_index.numpy(), g[f'u.{name}.index']) and split.data_index.shape[1] == 6, name
        split.eval_mode = name != 'trn'
        b = split[torch.arange(8)]
        want = {'user_id', 'in_item_id', 'in_rating', 'item_id', 'rating'} | ({'user_hist'} if name != 'trn' else set())
        assert set(b) == want and want <= set(g[f'u.{name}.keys'].tolist())
        for k in want:
            assert np.array_equal(b[k].numpy().astype(np.float32), g[f'u.{name}.{k}'].astype(np.float32)), (name, k)
    trn, val, _ = splits
    assert torch.equal(trn.data_index[:, 1:3], trn.data_index[:, 4:6])           # train: in_ = target = the train cut
    assert torch.equal(val.data_index[:, :3], trn.data_index[:, :3])             # valid: in_ = the train cut
    loader = trn.train_loader(batch_size=100, shuffle=True)
    assert len(loader) == 10 and set(next(iter(loader))) == {'user_id', 'in_item_id', 'in_rating', 'item_id', 'rating'}
    assert 'user_hist' in next(iter(val.eval_loader(batch_size=100)))


def test_users_without_a_valid_cut_are_dropped():
    users = np.repeat(np.arange(1, 7), [1, 1, 2, 12, 12, 12])
    items = np.arange(1, len(users) + 1)
    ds = UserDataset.from_interactions(users.astype(str), items.astype(str))
    trn, val, tst = ds.build(split_ratio=[0.8, 0.1, 0.1], shuffle=False)
    keep = (val.data_index[:, 5] > val.data_index[:, 4])
    assert bool(keep.all()) and len(trn) == len(val) == len(tst) < 6
    assert set(trn.data_index[:, 0].tolist()) == set(val.data_index[:, 0].tolist())


@pytest.mark.parametrize('mode', ['entry', 'user'])
def test_other_split_modes_raise(mode):
    users, items = np.repeat(np.arange(1, 4), 10), np.arange(1, 31)
    ds = UserDataset.from_interactions(users.astype(str), items.astype(str))
    with pytest.raises(NotImplementedError, match='user_entry'):
        ds.build(split_mode=mode)
