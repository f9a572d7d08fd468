"""CPU: the host side of ``BaseRetriever.fit`` -- the epoch driver both fit paths share, the one-batch-ahead driver, and the
classification of the stock configurations the fused kernels cover -- with fakes in place of the kernels."""
import pytest
import torch

from recstudio_amd.loss_func import BPRLoss, SampledSoftmaxLoss, SoftmaxLoss
from recstudio_amd.retriever import (BaseRetriever, _one_ahead, _stand_in_optimizer, _stock_forward, _stock_train_path)
from recstudio_amd.sampler import PopularSamplerModel, UniformSampler
from recstudio_amd.scorer import CosineScorer, EuclideanScorer, InnerProductScorer


# ------------------------------------------------------------------ the epoch driver
class Recorder:
    def __init__(self):
        self.lines = []

    def info(self, line):
        self.lines.append(line)


def run_epochs(metrics, train=None, eval_conf=None, scheduler=False, valid_time=False, log=True, validation=True):
    """``_run_epochs`` over a fake epoch (epoch k leaves k in the model's only buffer and reports the loss 1 / k) and a fake
    validation that replays ``metrics`` as ndcg@10; returns the model, the driver's result and what the hooks saw."""
    model = BaseRetriever({'train': dict({'epochs': len(metrics), 'early_stop_patience': 3}, **(train or {})),
                           'eval': dict({'val_metrics': ['ndcg', 'recall'], 'cutoff': [10, 20]}, **(eval_conf or {}))})
    model.register_buffer('mark', torch.zeros(()))
    model.logger = Recorder()
    seen = {'epochs': 0, 'validations': 0, 'restored': [], 'rates': [], 'lines': [], 'training': []}

    def train_epoch():
        seen['epochs'] += 1
        seen['training'].append(model.training)
        model.mark.fill_(seen['epochs'])
        return 1.0 / seen['epochs']

    def validate():
        out = {'ndcg@10': metrics[seen['epochs'] - 1], 'recall@10': 0.5}
        seen['validations'] += 1
        if valid_time:
            out['valid_time'] = 0.25
        return out

    sched = model._get_scheduler(_stand_in_optimizer(model.config['train']['learning_rate'])) if scheduler else None
    best = model._run_epochs(train_epoch, sched, validate if validation else None, on_lr=seen['rates'].append,
                             log=seen['lines'].append if log else None,
                             after_restore=lambda: seen['restored'].append(float(model.mark)))
    return model, best, seen


@pytest.mark.parametrize('mode, metrics, epochs, best, best_epoch', [
    # a tie is no improvement; the run ends after exactly three validations in a row that did not improve
    ('max', [0.1, 0.3, 0.3, 0.25, 0.29, 0.9, 0.9], 5, 0.3, 2),
    ('min', [0.5, 0.2, 0.3, 0.2, 0.4, 0.0, 0.0], 5, 0.2, 2),
    # an improvement starts the count again
    ('max', [0.1, 0.05, 0.05, 0.2, 0.1, 0.1, 0.1, 0.9], 7, 0.2, 4),
    # never three in a row: every epoch runs
    ('max', [0.1, 0.0, 0.0, 0.2, 0.0, 0.0], 6, 0.2, 4),
])
def test_epoch_driver_stops_on_patience_and_restores_the_best_state(mode, metrics, epochs, best, best_epoch):
    model, got, seen = run_epochs(metrics, train={'early_stop_mode': mode})
    assert model.val_metric == 'ndcg@10'
    assert got == best and seen['epochs'] == seen['validations'] == epochs == len(model.history)
    # the state of the best epoch is back, and the caller's hook ran once, after the restore
    assert float(model.mark) == best_epoch and seen['restored'] == [float(best_epoch)]
    assert all(seen['training'])
    assert [h['epoch'] for h in model.history] == list(range(epochs))
    assert [h['ndcg@10'] for h in model.history] == metrics[:epochs]
    assert [h['train_loss'] for h in model.history] == [1.0 / (k + 1) for k in range(epochs)]
    assert all(h['train_time'] >= 0 and 'valid_time' not in h and 'lr' not in h for h in model.history)
    assert model.logged_metrics == model.history[-1] and model.logged_metrics is not model.history[-1]
    assert seen['rates'] == []                                       # no scheduler: no rate to hand on


def test_epoch_driver_validates_every_val_n_epoch():
    model, got, seen = run_epochs([0.9, 0.1, 0.9, 0.2, 0.9, 0.3, 0.9], eval_conf={'val_n_epoch': 2}, valid_time=True)
    assert seen['epochs'] == 7 and seen['validations'] == 3 and got == 0.3
    assert ['ndcg@10' in h for h in model.history] == [False, True] * 3 + [False]
    # ``valid_time`` is the caller's: present exactly where its validation piece put it
    assert [h.get('valid_time') for h in model.history] == [None, 0.25] * 3 + [None]
    assert float(model.mark) == 6 and seen['restored'] == [6.0]


def test_epoch_driver_without_validation_data():
    model, got, seen = run_epochs([0.0] * 4, validation=False, train={'early_stop_patience': 0})
    assert got is None and seen['epochs'] == 4 and seen['validations'] == 0
    assert seen['restored'] == [] and float(model.mark) == 4          # nothing to restore, the hook stays uncalled
    assert all(set(h) == {'epoch', 'train_loss', 'train_time'} for h in model.history)


@pytest.mark.parametrize('name', ['exponential', 'onplateau'])
def test_epoch_driver_hands_the_schedulers_rate_on_after_every_epoch(name):
    metrics = [0.5] + [0.1] * 19                # the plateau scheduler (patience 10, factor 0.1) cuts the rate once
    model, _, seen = run_epochs(metrics, train={'scheduler': name, 'learning_rate': 0.1, 'early_stop_patience': 100},
                                scheduler=True)
    assert len(seen['rates']) == 20 and seen['rates'] == [h['lr'] for h in model.history]
    if name == 'exponential':
        assert seen['rates'] == pytest.approx([0.1 * 0.98 ** (k + 1) for k in range(20)], rel=1e-9)
    else:
        assert seen['rates'] == pytest.approx([0.1] * 11 + [0.01] * 9, rel=1e-9)


def test_epoch_driver_logs_through_the_callers_callback_only():
    model, _, seen = run_epochs([0.1, 0.2], valid_time=True)
    assert len(seen['lines']) == 2 and model.logger.lines == []
    assert seen['lines'][0].startswith('epoch=0 train_loss=1.0000 train_time=')
    assert seen['lines'][1].endswith('ndcg@10=0.2000 recall@10=0.5000 valid_time=0.2500')
    model, _, seen = run_epochs([0.1, 0.2], log=False)
    assert seen['lines'] == [] and model.logger.lines == [] and len(model.history) == 2


def test_cutoffs_are_a_list_whatever_the_config_holds():
    for cutoff, want in ((10, [10]), ([5, 10, 20], [5, 10, 20]), ([20], [20])):
        model = BaseRetriever({'eval': {'cutoff': cutoff}})
        assert model._cutoffs() == want


# ------------------------------------------------------------------ one batch ahead
@pytest.mark.parametrize('n, want', [(3, 'P0 P1 S0 P2 S1 S2'), (2, 'P0 P1 S0 S1'), (1, 'P0 S0'), (0, '')])
def test_one_ahead_issue_order(n, want):
    calls = []

    def prepare(b):
        calls.append(f'P{b}')
        return ('ticket', b)

    def step(b, ticket):
        assert ticket == ('ticket', b)                   # a batch is stepped with its own ticket
        calls.append(f'S{b}')
        return b * 10
    assert _one_ahead(iter(range(n)), step, prepare) == [b * 10 for b in range(n)]
    assert ' '.join(calls) == want


def test_one_ahead_switched_off_steps_in_order_without_tickets():
    calls = []

    def step(b, ticket):
        assert ticket is None
        calls.append(f'S{b}')
        return b
    assert _one_ahead(iter(range(3)), step) == [0, 1, 2] and calls == ['S0', 'S1', 'S2']
    assert _one_ahead(iter(()), step) == []


def test_one_ahead_takes_a_ticket_that_is_none():
    """What ``prepare`` returns is opaque: a falsy ticket must not make the driver prepare the batch again."""
    calls = []
    _one_ahead(iter(range(2)), lambda b, t: calls.append(f'S{b}'), lambda b: calls.append(f'P{b}'))
    assert calls == ['P0', 'P1', 'S0', 'S1']


# ------------------------------------------------------------------ which fused path a configuration takes
class MyBPR(BPRLoss):
    pass


class MySSM(SampledSoftmaxLoss):
    pass


class MySoftmax(SoftmaxLoss):
    pass


class MyInnerProduct(InnerProductScorer):
    pass


class MyUniform(UniformSampler):
    pass


SAMPLED = dict(loss=BPRLoss, scorer=InnerProductScorer, sampler=UniformSampler, item_embedding=True, n_item_fields=1,
               sampling_method='none', neg_count=64, dim=64, fused_ssm=True, fused_full_softmax=True)
FULL = dict(SAMPLED, loss=SoftmaxLoss, sampler=None, neg_count=0, dim=128)
SSM = dict(SAMPLED, loss=SampledSoftmaxLoss)

# (what differs from the base case, the path): one case at least for every condition that flips the answer
PATH_CASES = [
    (SAMPLED, {}, 'bpr'),
    (SAMPLED, {'sampler': PopularSamplerModel}, 'bpr'),
    (SAMPLED, {'neg_count': 128}, 'bpr'),
    (SAMPLED, {'dim': 32}, 'bpr'),                       # the autograd BPR path sets no width
    (SAMPLED, {'dim': 48}, 'bpr'),
    (SAMPLED, {'fused_ssm': False, 'fused_full_softmax': False}, 'bpr'),
    (SAMPLED, {'loss': MyBPR}, None),                    # ``type(...) is``: a subclass is another plugin
    (SAMPLED, {'scorer': MyInnerProduct}, None),
    (SAMPLED, {'scorer': CosineScorer}, None),           # fused forward, but not the one-launch loss
    (SAMPLED, {'scorer': EuclideanScorer}, None),
    (SAMPLED, {'sampler': MyUniform}, None),
    (SAMPLED, {'sampling_method': 'dns'}, None),
    (SAMPLED, {'neg_count': 63}, None),
    (SAMPLED, {'neg_count': 65}, None),
    (SAMPLED, {'neg_count': 0}, None),
    (SAMPLED, {'neg_count': None}, None),
    (SAMPLED, {'neg_count': [64, 64]}, None),
    (SAMPLED, {'neg_count': (128, 64)}, None),
    (SAMPLED, {'item_embedding': False, 'dim': None}, None),
    (SAMPLED, {'n_item_fields': 2}, None),
    (SAMPLED, {'loss': SoftmaxLoss}, None),              # full softmax is the path WITHOUT a sampler
    (SSM, {}, 'ssm'),
    (SSM, {'dim': 32}, 'ssm'),
    (SSM, {'dim': 256}, 'ssm'),
    (SSM, {'neg_count': 256, 'sampler': PopularSamplerModel}, 'ssm'),
    (SSM, {'dim': 48}, None),
    (SSM, {'dim': 192}, None),
    (SSM, {'dim': 512}, None),
    (SSM, {'fused_ssm': False}, None),
    (SSM, {'loss': MySSM}, None),
    (SSM, {'neg_count': 63}, None),
    (SSM, {'neg_count': [64, 64]}, None),
    (SSM, {'scorer': CosineScorer}, None),
    (SSM, {'sampler': MyUniform}, None),
    (SSM, {'sampling_method': 'sir'}, None),
    (SSM, {'fused_full_softmax': False}, 'ssm'),
    (FULL, {}, 'full_softmax'),
    (FULL, {'dim': 32}, 'full_softmax'),
    (FULL, {'dim': 48}, 'full_softmax'),
    (FULL, {'dim': 192}, None),
    (FULL, {'dim': 129}, None),
    (FULL, {'fused_full_softmax': False}, None),
    (FULL, {'fused_ssm': False}, 'full_softmax'),
    (FULL, {'loss': MySoftmax}, None),
    (FULL, {'loss': BPRLoss}, None),
    (FULL, {'scorer': CosineScorer}, None),
    (FULL, {'scorer': MyInnerProduct}, None),
    (FULL, {'item_embedding': False, 'dim': None}, None),
    (FULL, {'n_item_fields': 2}, None),
    (FULL, {'sampler': UniformSampler}, None),
    (FULL, {'sampling_method': 'dns'}, 'full_softmax'),  # neither looked at without a sampler
    (FULL, {'neg_count': [64, 64]}, 'full_softmax'),
]


@pytest.mark.parametrize('base, change, want', PATH_CASES)
def test_stock_train_path(base, change, want):
    assert _stock_train_path(**dict(base, **change)) == want


@pytest.mark.parametrize('change, want', [
    ({}, True), ({'scorer': CosineScorer}, True), ({'scorer': EuclideanScorer}, True), ({'sampler': PopularSamplerModel}, True),
    ({'sampler': None}, True), ({'neg_count': 63}, True), ({'neg_count': None}, True), ({'loss': MyBPR, 'dim': 48}, True),
    ({'scorer': MyInnerProduct}, False), ({'sampler': MyUniform}, False), ({'sampling_method': 'dns'}, False),
    ({'neg_count': [64, 64]}, False), ({'neg_count': (64, 64)}, False), ({'item_embedding': False, 'dim': None}, False),
    ({'n_item_fields': 2}, False), ({'n_item_fields': 0}, False),
])
def test_stock_forward(change, want):
    assert bool(_stock_forward(**dict(SAMPLED, **change))) is want


def stock_model(train=None, **attrs):
    """A BPR two-tower model assembled by hand on the CPU (no dataset, no kernels): what ``_init_model`` would leave."""
    model = BaseRetriever({'train': dict({'negative_count': 64}, **(train or {}))},
                          item_encoder=torch.nn.Embedding(11, 64, padding_idx=0), query_encoder=torch.nn.Embedding(7, 64, padding_idx=0),
                          loss=BPRLoss(), sampler=UniformSampler(10))
    model.fiid, model.fuid, model.item_fields, model.neg_count = 'item_id', 'user_id', {'item_id'}, 64
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def test_fused_train_path_of_a_model_and_a_batch():
    one, many = {'item_id': torch.ones(4, dtype=torch.int64)}, {'item_id': torch.ones(4, 3, dtype=torch.int64)}
    model = stock_model()
    assert model._fused_ok() and model._fused_train_path() == model._fused_train_path(one) == 'bpr'
    assert model._fused_train_path(many) is None                        # several positives per query: the per-plugin path
    assert stock_model(loss_fn=SampledSoftmaxLoss())._fused_train_path(one) == 'ssm'
    assert stock_model(train={'fused_ssm': False}, loss_fn=SampledSoftmaxLoss())._fused_train_path(one) is None
    assert stock_model(loss_fn=MyBPR())._fused_train_path(one) is None
    assert stock_model(neg_count=63)._fused_train_path(one) is None
    assert stock_model(train={'sampling_method': 'dns'})._fused_train_path(one) is None
    wide = stock_model(item_encoder=torch.nn.Embedding(11, 192), loss_fn=SoftmaxLoss(), sampler=None)
    assert wide._fused_ok() and wide._fused_train_path(one) is None
    full = stock_model(loss_fn=SoftmaxLoss(), sampler=None)
    assert full._fused_train_path(one) == 'full_softmax' and full._fused_train_path(many) is None
    tower = stock_model(item_encoder=torch.nn.Sequential(torch.nn.Embedding(11, 64)))
    assert not tower._fused_ok() and tower._fused_train_path(one) is None


def test_query_source():
    model = stock_model()
    ids = torch.tensor([1, 2, 2], dtype=torch.int64)
    src, idx = model._query_source(ids)
    assert src is model.query_encoder.weight and idx is ids               # the kernel gathers the user rows
    for feat, kw in ((ids, {'gather_in_kernel': False}), (ids.view(3, 1), {})):
        src, idx = model._query_source(feat, **kw)
        assert idx is None and torch.equal(src, model.query_encoder(feat))
    model.query_encoder = torch.nn.Sequential(model.query_encoder)         # any other tower: encoded queries
    src, idx = model._query_source(ids)
    assert idx is None and src.shape == (3, 64)


def test_fused_optimizer_needs_the_stock_configuration():
    assert stock_model()._fused_optimizer_step({'fused_optimizer': None}) is None
    for bad in (dict(loss_fn=MyBPR()), dict(neg_count=63), dict(query_encoder=torch.nn.Sequential(torch.nn.Embedding(7, 64))),
                dict(item_encoder=torch.nn.Embedding(11, 32), query_encoder=torch.nn.Embedding(7, 32))):
        with pytest.raises(NotImplementedError, match='stock BPR two-tower'):
            stock_model(**bad)._fused_optimizer_step({'fused_optimizer': 'sgd'})
    for conf in ({'weight_decay': 0.01}, {'grad_clip_norm': 1.0}):
        with pytest.raises(NotImplementedError, match='stock BPR two-tower'):
            stock_model()._fused_optimizer_step(dict({'fused_optimizer': 'adam'}, **conf))
    with pytest.raises(ValueError, match="'sgd' or 'adam'"):
        stock_model()._fused_optimizer_step({'fused_optimizer': 'adagrad'})
