"""CPU: the product loaders (recstudio_amd/dataset.py) against fixtures recorded from the
reference's TripletDataset / SeqDataset on its bundled ml-100k demo file."""
import hashlib
import os
import shutil

import numpy as np
import torch

from recstudio_amd.dataset import DataSampler, SeqDataset, SortedDataSampler, TripletDataset, synthetic_interactions


def seed_everything(seed):
    """What recstudio.utils.seed_everything does for the host generators (utils.py:374-377)."""
    import random
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def make(cls, g, **cfg):
    conf = {'low_rating_thres': 3.0}
    conf.update(cfg)
    ds = cls('ml-100k', conf, _interactions=(g['raw_user'].astype(str), g['raw_item'].astype(str),
                                             g['raw_rating'].astype(np.float64), g['raw_time'].astype(np.float64)))
    return ds


def test_triplet_dataset_matches_reference(golden):
    g = golden('data_ml100k')
    seed_everything(2022)
    ds = make(TripletDataset, g)
    assert (ds.num_users, ds.num_items) == (int(g['t_num_users']), int(g['t_num_items'])) == (944, 1575)
    trn, val, tst = ds.build(split_ratio=[0.8, 0.1, 0.1], shuffle=True, split_mode='user_entry')
    assert trn.num_inters == int(g['t_num_inter'])
    assert np.array_equal(trn.inter_feat['user_id'].numpy(), g['t_inter_user'])
    assert np.array_equal(trn.inter_feat['item_id'].numpy(), g['t_inter_item'])     # incl. the seeded per-user shuffle
    assert np.array_equal(trn.inter_feat['rating'].numpy().astype(np.int8), g['t_inter_rating'])
    assert np.array_equal(trn.data_index.numpy(), g['t_train_index']) and len(trn) == 66868
    assert np.array_equal(val.data_index.numpy(), g['t_val_index'])
    assert np.array_equal(tst.data_index.numpy(), g['t_test_index'])
    assert np.array_equal(trn.item_freq.numpy(), g['t_item_freq'])
    assert np.array_equal(trn.user_count.numpy(), g['t_user_count'])
    assert tuple(trn.user_hist.shape) == tuple(g['t_user_hist_shape'])
    assert np.array_equal(trn.user_hist[:8].numpy(), g['t_user_hist_head'])
    assert tuple(tst.user_hist.shape) == tuple(g['t_test_user_hist_shape'])
    assert np.array_equal(tst.user_hist[:8].numpy(), g['t_test_user_hist_head'])
    assert np.array_equal(tst.user_count.numpy(), g['t_test_user_count'])
    trn.drop_feat(trn.use_field)
    loader = trn.train_loader(batch_size=512, shuffle=False)
    assert len(loader) == int(g['t_n_train_batches']) == 131
    for i, b in zip(range(2), loader):
        assert sorted(b) == ['item_id', 'rating', 'user_id']
        assert np.array_equal(b['user_id'].numpy(), g[f't_trainbatch{i}_user'])
        assert np.array_equal(b['item_id'].numpy(), g[f't_trainbatch{i}_item'])
        assert np.array_equal(b['rating'].numpy(), g[f't_trainbatch{i}_rating']) and b['rating'].dtype == torch.float32
    ev = val.eval_loader(batch_size=20)
    assert len(ev) == int(g['t_n_val_batches'])
    for i, b in zip(range(2), ev):
        for k in ('user_id', 'item_id', 'rating', 'user_hist'):
            assert np.array_equal(b[k].numpy(), g[f't_valbatch{i}_{k}']), k


def test_seq_dataset_matches_reference(golden):
    g = golden('data_ml100k')
    seed_everything(2022)
    sq = make(SeqDataset, g, max_seq_len=50)
    strn, sval, stst = sq.build(split_ratio=2, split_mode='user_entry')
    assert (sq.num_users, sq.num_items, sq.num_inters) == (int(g['s_num_users']), int(g['s_num_items']), int(g['s_num_inter']))
    assert [len(strn), len(sval), len(stst)] == g['s_sizes'].tolist()
    assert np.array_equal(strn.inter_feat['item_id'].numpy(), g['s_inter_item'])
    assert np.array_equal(strn.data_index[:300].numpy(), g['s_train_index_head'])
    assert np.array_equal(strn.data_index[-300:].numpy(), g['s_train_index_tail'])
    assert np.array_equal(sval.data_index.numpy(), g['s_val_index'])
    assert np.array_equal(stst.data_index.numpy(), g['s_test_index'])
    assert np.array_equal(strn.item_freq.numpy(), g['s_item_freq'])
    strn.drop_feat(strn.use_field)
    for i, b in zip(range(2), strn.train_loader(batch_size=64, shuffle=False)):
        assert sorted(b) == g[f's_trainbatch{i}_keys'].tolist()
        for k in ('user_id', 'seqlen', 'in_item_id', 'item_id', 'in_rating', 'rating'):
            assert np.array_equal(b[k].numpy(), g[f's_trainbatch{i}_{k}']), k
    flat, start, end = strn.segments(torch.arange(5))
    assert torch.equal(flat[start[3]:end[3]], strn[torch.arange(5)]['in_item_id'][3, :int(end[3] - start[3])])


def test_samplers_and_synthetic_stream():
    class Src:
        sample_length = torch.tensor([5, 1, 3, 3, 9, 2, 7])

        def __len__(self):
            return 7
    torch.manual_seed(3)
    a = list(DataSampler(Src(), 3, shuffle=True))
    assert sorted(torch.cat(a).tolist()) == list(range(7)) and [len(x) for x in a] == [3, 3, 1]
    assert [len(x) for x in DataSampler(Src(), 3, shuffle=False, drop_last=True)] == [3, 3]
    b = torch.cat(list(SortedDataSampler(Src(), 3)))
    assert Src.sample_length[b].tolist() == sorted(Src.sample_length.tolist())
    u, i = synthetic_interactions(50, 200, 5000, seed=2)
    assert u.min() >= 1 and u.max() <= 50 and i.min() >= 1 and i.max() <= 200
    u2, i2 = synthetic_interactions(50, 200, 5000, seed=2)
    assert np.array_equal(i, i2)
    cnt = np.bincount(i, minlength=201)
    assert cnt.max() > 20 * np.median(cnt[1:])          # Zipf head
    ds = TripletDataset.from_interactions(u, i)
    trn, val, tst = ds.build()
    assert len(trn) + sum(int(x) for x in (val.data_index[:, 2] - val.data_index[:, 1])) + \
        sum(int(x) for x in (tst.data_index[:, 2] - tst.data_index[:, 1])) == ds.num_inters


def test_flat_cache_round_trip(golden, tmp_path):
    """save_cache / load_cache (one flat .npz instead of the reference's pickled object): the reloaded dataset
    builds the same splits and batches."""
    g = golden('data_ml100k')
    for cls, cfg, kw in ((TripletDataset, {}, dict(split_ratio=[0.8, 0.1, 0.1], shuffle=True)),
                         (SeqDataset, {'max_seq_len': 50}, dict(split_ratio=2))):
        ds = make(cls, g, **cfg)
        path = tmp_path / f'{cls.__name__}.npz'
        ds.save_cache(path)
        ds2 = cls.load_cache(path)
        assert type(ds2) is cls and ds2.num_users == ds.num_users and ds2.num_items == ds.num_items
        for k in ds.inter_feat:
            assert torch.equal(ds.inter_feat[k], ds2.inter_feat[k]) and ds.inter_feat[k].dtype == ds2.inter_feat[k].dtype
        assert list(ds.field2tokens[ds.fiid][:5]) == list(ds2.field2tokens[ds2.fiid][:5])
        seed_everything(2022)
        a = ds.build(**kw)
        seed_everything(2022)
        b = ds2.build(**kw)
        for x, y in zip(a, b):
            assert torch.equal(x.data_index, y.data_index)
        ba = next(iter(a[0].train_loader(64, shuffle=False)))
        bb = next(iter(b[0].train_loader(64, shuffle=False)))
        assert sorted(ba) == sorted(bb) and all(torch.equal(ba[k], bb[k]) for k in ba)


def _write_atomic(tmp_path, g, rows=None, user_feat=True):
    """The fixture's raw interaction columns written back in RecStudio's atomic-file layout (tab-separated,
    one header row -- recstudio/data/config/ml-100k.yaml, dataset_demo/ml-100k/ml-100k.inter)."""
    sel = slice(None) if rows is None else rows
    u, i = g['raw_user'][sel], g['raw_item'][sel]
    r, t = g['raw_rating'][sel], g['raw_time'][sel]
    with open(tmp_path / 'demo.inter', 'w') as f:
        f.write('user_id\titem_id\trating\ttimestamp\n')
        for a, b, c, d in zip(u, i, r, t):
            f.write(f'{a}\t{b}\t{int(c)}\t{int(d)}\n')
    if user_feat:
        with open(tmp_path / 'demo.user', 'w') as f:
            f.write('user_id\tage\tgender\n')
            for a in sorted(set(u.tolist()) | {99999}):        # one user without interactions
                f.write(f'{a}\t30\tM\n')
    return {'data_dir': str(tmp_path), 'inter_feat_name': 'demo.inter', 'inter_feat_header': 0, 'field_separator': '\t',
            'user_feat_name': ['demo.user'] if user_feat else None, 'user_feat_header': 0, 'low_rating_thres': 3.0}


def test_atomic_file_reader_equals_injected_interactions(golden, tmp_path):
    """TripletDataset built by PARSING atomic files (recstudio/data/dataset.py:945-974 `build` <- `_load_all_data`) ==
    the dataset built from the same columns handed over in memory, which the tests above pin to the reference: ids,
    splits, item_freq, first batch."""
    g = golden('data_ml100k')
    cfg = _write_atomic(tmp_path, g, user_feat=False)
    seed_everything(2022)
    a = TripletDataset('demo', cfg)
    seed_everything(2022)
    b = make(TripletDataset, g)
    assert (a.num_users, a.num_items) == (b.num_users, b.num_items) == (944, 1575)
    for f in ('user_id', 'item_id', 'rating'):
        assert torch.equal(a.inter_feat[f], b.inter_feat[f]), f
    seed_everything(2022)
    ta, va, _ = a.build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)
    seed_everything(2022)
    tb, vb, _ = b.build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)
    assert torch.equal(ta.data_index, tb.data_index) and torch.equal(va.data_index, vb.data_index)
    assert torch.equal(ta.item_freq, tb.item_freq) and np.array_equal(ta.item_freq.numpy(), g['t_item_freq'])
    ba, bb = next(iter(ta.train_loader(512, shuffle=False))), next(iter(tb.train_loader(512, shuffle=False)))
    assert all(torch.equal(ba[k], bb[k]) for k in bb)
    # a user-feature file adds the users that never interacted to the id space (the reference maps ids over the
    # union of the feature files); rows with missing values are dropped
    cfg2 = _write_atomic(tmp_path, g, rows=slice(0, 3000), user_feat=True)
    with open(tmp_path / 'demo.inter', 'a') as f:
        f.write('7\t\t5\t1\n')
    c = TripletDataset('demo', cfg2)
    d = TripletDataset('demo', dict(cfg2, user_feat_name=None))
    # (users whose only interactions fall below low_rating_thres stay in the id space through the feature file)
    assert c.num_users == len(set(g['raw_user'][:3000].tolist())) + 1 + 1 and c.num_users > d.num_users
    assert c.num_items == d.num_items
    assert len(c.inter_feat['user_id']) == len(d.inter_feat['user_id'])


# sha256 of the reference's recstudio/dataset_demo/ml-100k/ml-100k.inter
ML100K_INTER_SHA256 = 'ecb4025ec09d52830e65854de08fd07a79ff7bb9201f7067d753c2f0516e5674'


def test_atomic_file_reader_on_the_reference_demo_files(golden, tmp_path):
    """The reference's own bundled ml-100k atomic files through the product reader == the recorded fixture.  The
    interaction file is rebuilt from the fixture's raw columns, byte for byte (its digest is the reference file's); the
    user file is the reference's, kept as tests/golden/ml-100k.user."""
    g = golden('data_ml100k')
    _write_atomic(tmp_path, g, user_feat=False)
    (tmp_path / 'demo.inter').rename(tmp_path / 'ml-100k.inter')
    assert hashlib.sha256((tmp_path / 'ml-100k.inter').read_bytes()).hexdigest() == ML100K_INTER_SHA256
    shutil.copy(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ml-100k.user'), tmp_path)
    cfg = {'data_dir': str(tmp_path), 'inter_feat_name': 'ml-100k.inter',
           'inter_feat_header': 0, 'field_separator': '\t', 'user_feat_name': ['ml-100k.user'], 'user_feat_header': 0,
           'low_rating_thres': 3.0}
    seed_everything(2022)
    ds = TripletDataset('ml-100k', cfg)
    assert (ds.num_users, ds.num_items) == (944, 1575)
    trn, _, _ = ds.build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)
    assert np.array_equal(trn.inter_feat['user_id'].numpy(), g['t_inter_user'])
    assert np.array_equal(trn.inter_feat['item_id'].numpy(), g['t_inter_item'])
    assert np.array_equal(trn.item_freq.numpy(), g['t_item_freq'])
