"""CPU: what the split of retriever.py into family modules and the one defaults rule (``config_defaults``) must keep.
(1) Every class resolves every recorded input config to exactly what it resolved to before the defaults moved
(tests/golden/model_configs.json, tools/make_golden_model_configs.py), and instances share no list.  (2) Every module imports on
its own in a fresh interpreter and every name the package and ``retriever`` exported keeps resolving, to the same object.
(3) A plain SASRecQueryEncoder takes CPU tensors like the other towers and computes the stock op sequence."""
import copy
import json
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

with open(os.path.join(GOLDEN, 'model_configs.json')) as f:
    CASES = json.load(f)
CLASSES = ('BaseRetriever', 'BPR', 'LightGCN', 'SGL', 'SimGCL', 'NGCF', 'SASRec', 'CL4SRec', 'GRU4Rec', 'NARM', 'STAMP', 'HGN',
           'MultiDAE', 'MultiVAE')
# what recstudio_amd/__init__.py took from retriever, and retriever.__all__, before the split
PACKAGE_NAMES = ('BaseRetriever', 'TwoTowerRecommender', 'ItemTowerRecommender', 'BPR', 'SASRec', 'LightGCN', 'SGL', 'SimGCL', 'NGCF',
                 'CL4SRec', 'GRU4Rec', 'NARM', 'STAMP', 'HGN', 'HGNQueryEncoder', 'MultiDAE', 'MultiVAE', 'MultiDAEQueryEncoder',
                 'MultiVAEQueryEncoder', 'default_config', 'seed_everything')
RETRIEVER_ALL = ['BaseRetriever', 'TwoTowerRecommender', 'ItemTowerRecommender', 'BPR', 'SASRec', 'CL4SRec', 'GRU4Rec', 'NARM',
                 'STAMP', 'HGN', 'MultiDAE', 'MultiVAE', 'LightGCN', 'SGL', 'SimGCL', 'default_config', 'seed_everything']
HOMES = {'models_graph': ('LightGCN', 'SGL', 'SimGCL', 'NGCF'),
         'models_seq': ('SASRecQueryEncoder', 'GRU4RecQueryEncoder', 'NARMQueryEncoder', 'STAMPQueryEncoder', 'CaserQueryEncoder',
                        'HGNQueryEncoder', 'SASRec', 'CL4SRec', 'GRU4Rec', 'NARM', 'STAMP', 'HGN', 'FUSED_ATTENTION_POOL_DEFAULT',
                        'FUSED_INFONCE_DEFAULT', 'FUSED_GATING_DEFAULT'),
         'models_ae': ('MultiDAEQueryEncoder', 'MultiVAEQueryEncoder', 'MultiDAE', 'MultiVAE', 'FUSED_BAG_DEFAULT')}


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    return recstudio_amd


def test_the_recording_covers_every_class_and_collision():
    seen = {(c['class'], c['case']) for c in CASES}
    assert {(name, case) for name in CLASSES for case in ('none', 'all_changed')} <= seen
    assert {('CL4SRec', 'hidden_size_only'), ('CL4SRec', 'layer_num_only'), ('NGCF', 'layer_size_only'),
            ('NGCF', 'l2_reg_weight_only'), ('MultiDAE', 'embed_dim_only'), ('MultiVAE', 'embed_dim_only'),
            ('SimGCL', 'batch_size_only')} <= seen


@pytest.mark.parametrize('case', CASES, ids=[f"{c['class']}-{c['case']}" for c in CASES])
def test_resolved_config_is_the_recorded_one(ra, case):
    given = copy.deepcopy(case['config'])
    model = getattr(ra, case['class'])(given)
    assert model.config == case['resolved']
    assert model.embed_dim == case['embed_dim'] == model.config['model']['embed_dim']
    assert given == case['config']                                  # the caller's config is read, not written
    if case['case'] == 'all_changed':                               # the caller won on every key it set
        for group, values in case['config'].items():
            for key, value in values.items():
                if (case['class'], key) != ('NGCF', 'n_layers'):    # derived from layer_size, whoever sets it
                    assert model.config[group][key] == value, (group, key)


def test_the_collisions_say_what_they_should(ra):
    got = {(c['class'], c['case']): c['resolved'] for c in CASES}
    assert got['CL4SRec', 'hidden_size_only']['model']['hidden_size'] == 32
    m = got['CL4SRec', 'layer_num_only']['model']
    assert (m['hidden_size'], m['layer_num']) == (64, 3)
    m = got['NGCF', 'layer_size_only']['model']
    assert (m['n_layers'], m['mess_dropout'], m['l2_reg_weight']) == (1, [0.1], 1e-5)
    assert got['NGCF', 'l2_reg_weight_only']['model']['l2_reg_weight'] == 0.5
    assert 'dropout' not in got['MultiVAE', 'none']['model'] and 'dropout_rate' not in got['MultiDAE', 'none']['model']
    assert got['SimGCL', 'batch_size_only']['train']['batch_size'] == 77


@pytest.mark.parametrize('name', CLASSES)
def test_instances_share_no_list(ra, name):
    cls = getattr(ra, name)
    first, want = cls(), copy.deepcopy(cls().config)
    for values in first.config.values():
        for value in values.values():
            if isinstance(value, list):
                value.append('x')
    assert cls().config == want
    assert all('x' not in v for klass in cls.__mro__ for g in vars(klass).get('config_defaults', {}).values()
               for v in g.values() if isinstance(v, list))


def test_ngcf_layer_size_is_not_shared(ra):
    ra.NGCF().config['model']['layer_size'].append(8)
    assert ra.NGCF().config['model']['layer_size'] == [64, 64, 64, 64] == ra.NGCF.config_defaults['model']['layer_size']


@pytest.mark.parametrize('module', ['data_augmentation', 'gather', 'models_graph', 'models_seq', 'models_ae', 'retriever'])
def test_module_imports_on_its_own(module):
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = subprocess.run([sys.executable, '-c', f'import recstudio_amd.{module}'], cwd=ROOT, env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


def test_gather_imports_torch_and_ops_only():
    with open(os.path.join(ROOT, 'recstudio_amd', 'gather.py')) as f:
        imports = set(re.findall(r'^(?:import|from) .*$', f.read(), flags=re.M))
    assert imports == {'import torch', 'from . import ops'}
    with open(os.path.join(ROOT, 'recstudio_amd', 'data_augmentation.py')) as f:
        assert not re.search(r'^\s+from \.retriever import', f.read(), flags=re.M)


def test_every_name_keeps_resolving(ra):
    from recstudio_amd import gather, models_ae, models_graph, models_seq, retriever
    assert retriever.__all__ == RETRIEVER_ALL
    for name in PACKAGE_NAMES:
        assert getattr(ra, name) is getattr(retriever, name), name
    for name in RETRIEVER_ALL:
        assert hasattr(retriever, name), name
    modules = {'models_graph': models_graph, 'models_seq': models_seq, 'models_ae': models_ae}
    for module, names in HOMES.items():
        for name in names:
            assert getattr(retriever, name) is getattr(modules[module], name), name
    assert retriever.SASRecQueryEncoder is models_seq.SASRecQueryEncoder
    assert retriever.TwoTowerRecommender is retriever.ItemTowerRecommender is retriever.BaseRetriever
    for name in ('_EmbedFn', '_SegEmbedFn', '_embedding_grad', '_history_rows', '_last_position'):
        assert hasattr(gather, name), name
    for name in ('_device_init_block', '_init_weights', '_stock_forward', '_stock_train_path', '_stand_in_optimizer', '_one_ahead',
                 '_with_next', '_above_second_stream'):
        assert hasattr(retriever, name), name


def test_the_sequence_base(ra):
    from recstudio_amd import models_seq
    for name in ('SASRec', 'CL4SRec', 'GRU4Rec', 'NARM', 'STAMP', 'HGN'):
        cls = getattr(ra, name)
        assert issubclass(cls, models_seq.SeqRetriever) and cls._get_dataset_class() is ra.SeqDataset
        batch = {'in_item_id': torch.zeros(1, 2), 'seqlen': torch.ones(1)}
        assert cls()._get_query_feat(batch) is batch
    assert not issubclass(ra.MultiDAE, models_seq.SeqRetriever) and ra.MultiDAE._get_dataset_class() is ra.UserDataset
    assert ra.MultiVAE._get_dataset_class() is ra.UserDataset and ra.BPR._get_dataset_class() is ra.TripletDataset
    batch = {'in_item_id': torch.zeros(1, 2)}
    assert ra.MultiDAE()._get_query_feat(batch) is batch and ra.MultiVAE()._get_query_feat(batch) is batch


@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
def test_plain_sasrec_tower_takes_cpu_tensors(train):
    """No fused attention, no mask token: before the towers shared one gather this setting alone refused CPU tensors."""
    from recstudio_amd.models_seq import SASRecQueryEncoder
    torch.manual_seed(3)
    B, L, N, D = 5, 8, 50, 16
    item = torch.nn.Embedding(N, D, padding_idx=0)
    enc = SASRecQueryEncoder('item_id', D, L, 2, 32, 0.0, 'gelu', 1e-12, 2, item).train(train)
    seqlen = torch.tensor([1, 3, 8, 8, 5])
    hist = torch.randint(1, N, (B, L)) * (torch.arange(L).unsqueeze(0) < seqlen.unsqueeze(1))
    got = enc({'in_item_id': hist, 'seqlen': seqlen})
    got.sum().backward()
    grad, item.weight.grad = item.weight.grad, None

    rows = F.embedding(hist, item.weight, padding_idx=0) + enc.position_emb(torch.arange(L).unsqueeze(0).expand(B, L))
    out = enc.transformer_layer(enc.dropout(rows), mask=torch.triu(torch.ones(L, L, dtype=torch.bool), 1),
                                src_key_padding_mask=hist == 0)
    want = out.gather(1, (seqlen - 1).view(-1, 1, 1).expand(-1, 1, D)).squeeze(1)
    want.sum().backward()
    assert got.shape == (B, D) and torch.equal(got, want) and torch.equal(grad, item.weight.grad)
