"""Records tests/golden/model_configs.json: the resolved ``config`` and ``embed_dim`` of every retriever class, per case.  It was
run on the commit BEFORE the models' defaults moved to ``config_defaults`` (docs/HISTORY.md), so the file pins what every
constructor resolved to then; tests/test_model_configs.py replays the recorded input configs and asserts exact equality.  Run by
hand on the CPU (no device, no built library is needed: a constructor touches neither):

    python tools/make_golden_model_configs.py

CASES per class.  ``none``: no config.  ``all_changed``: every key of the class's resolved config (a superset of the keys its
defaults touch) set to a different value of the same type -- int + 1, float / 2, bool negated, str + '_x', a list shortened by its
last element (doubled when it has one); keys whose value is ``None`` carry no type and stay (``train.ann`` among them, which must
stay ``None``).  NGCF's values are tied together by its constructor's checks, so its ``all_changed`` case states the tied ones by
hand.  Then the collision cases, where a derived class's default, its parent's and the caller's meet on one key.  Data only."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ('BaseRetriever', 'BPR', 'LightGCN', 'SGL', 'SimGCL', 'NGCF', 'SASRec', 'CL4SRec', 'GRU4Rec', 'NARM', 'STAMP', 'HGN',
           'MultiDAE', 'MultiVAE')
COLLISIONS = (
    ('CL4SRec', 'hidden_size_only', {'model': {'hidden_size': 32}}),
    ('CL4SRec', 'layer_num_only', {'model': {'layer_num': 3}}),
    ('NGCF', 'layer_size_only', {'model': {'layer_size': [64, 32]}}),
    ('NGCF', 'l2_reg_weight_only', {'model': {'l2_reg_weight': 0.5}}),
    ('MultiDAE', 'embed_dim_only', {'model': {'embed_dim': 48}}),
    ('MultiVAE', 'embed_dim_only', {'model': {'embed_dim': 48}}),
    ('SimGCL', 'batch_size_only', {'train': {'batch_size': 77}}),
)
# (embed_dim == layer_size[0], one mess_dropout per layer, sum(layer_size) <= 256)
TIED = {'NGCF': {'model': {'embed_dim': 32, 'layer_size': [32, 16, 16], 'mess_dropout': [0.2, 0.3], 'n_layers': 7}}}


def changed(value):
    if isinstance(value, bool):
        return not value
    if isinstance(value, int):
        return value + 1
    if isinstance(value, float):
        return value / 2
    if isinstance(value, str):
        return value + '_x'
    if isinstance(value, list):
        return value[:-1] if len(value) > 1 else value + value
    return value


def all_changed(cls):
    config = {group: {k: changed(v) for k, v in values.items()} for group, values in cls().config.items()}
    for group, values in TIED.get(cls.__name__, {}).items():
        config[group].update(values)
    return config


def record(cls, case, config):
    model = cls(copy.deepcopy(config))
    return {'class': cls.__name__, 'case': case, 'config': config, 'resolved': model.config, 'embed_dim': model.embed_dim}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'model_configs.json'))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import recstudio_amd as ra

    cases = []
    for name in CLASSES:
        cls = getattr(ra, name)
        cases.append(record(cls, 'none', None))
        cases.append(record(cls, 'all_changed', all_changed(cls)))
    cases += [record(getattr(ra, name), case, config) for name, case, config in COLLISIONS]
    with open(args.out, 'w') as f:                                             # one case per line
        f.write('[\n' + ',\n'.join(json.dumps(case, sort_keys=True) for case in cases) + '\n]\n')
    print(args.out, os.path.getsize(args.out), 'bytes;', len(cases), 'cases')


if __name__ == '__main__':
    main()
