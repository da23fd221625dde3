"""Minimal configuration + factory layer so the reference's experiment YAMLs drive this package unmodified
(`configs/scannet/mvpnet_3d_unet_resnet34_pn2ssg.yaml`, `configs/scannet/3d_baselines/pn2ssg_chunk.yaml`,
`configs/scannet/unet_resnet34.yaml`).

The reference uses yacs (absent here): defaults in `common/config/base.py:10-137`, task defaults in
`mvpnet/config/mvpnet_3d.py:6-80` / `mvpnet/config/sem_seg_3d.py` / `mvpnet/config/sem_seg_2d.py`, `purge_cfg` in
`common/config/__init__.py:4-17`, factories in `mvpnet/models/build.py:8-47` and
`common/solver/build.py:7-41`.  This is a PyYAML + `ast.literal_eval` work-alike of exactly what those
need: nested attribute access, defaults, `merge_from_file` / `merge_from_list`, tuples written as strings
("(160, 120)") evaluated like yacs does, and TYPE-keyed purge.  The default trees below are pinned key by key
against the reference's own config modules (tests/golden/config_defaults.json, dumped by importing them with a
dict stand-in for yacs: tests/golden/make_golden.py::gen_config_defaults).
"""
import ast
import copy

import yaml


class CfgNode(dict):
    """dict with attribute access (the subset of yacs.config.CfgNode the reference relies on)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        self[name] = value

    def clone(self):
        return copy.deepcopy(self)

    @staticmethod
    def _convert(value):
        if isinstance(value, dict):
            node = CfgNode()
            for k, v in value.items():
                node[k] = CfgNode._convert(v)
            return node
        if isinstance(value, str):  # yacs literal_evals strings: "(160, 120)" -> (160, 120)
            try:
                return ast.literal_eval(value)
            except (ValueError, SyntaxError):
                return value
        if isinstance(value, list):
            return tuple(CfgNode._convert(v) for v in value)
        return value

    def merge(self, other):
        for k, v in other.items():
            if isinstance(v, dict) and isinstance(self.get(k), dict):
                self[k].merge(v)
            else:
                self[k] = v
        return self

    def merge_from_file(self, path):
        with open(path) as f:
            return self.merge(CfgNode._convert(yaml.safe_load(f) or {}))

    def merge_from_text(self, text):
        return self.merge(CfgNode._convert(yaml.safe_load(text) or {}))

    def merge_from_list(self, opts):
        """['OPTIMIZER.BASE_LR', '0.001', ...] like the reference CLI overrides (train_mvpnet_3d.py:301-305)."""
        assert len(opts) % 2 == 0
        for key, value in zip(opts[0::2], opts[1::2]):
            node = self
            parts = key.split('.')
            for p in parts[:-1]:
                node = node.setdefault(p, CfgNode())
            node[parts[-1]] = CfgNode._convert(value)
        return self


def _base():
    """common/config/base.py:10-137 (the keys this package reads; the YAML may add others)."""
    return CfgNode._convert({
        'TASK': '', 'AUTO_RESUME': True, 'RESUME_STATES': True, 'RESUME_PATH': '',
        'MODEL': {'TYPE': ''}, 'DATASET': {'TYPE': ''}, 'DATALOADER': {'NUM_WORKERS': 0, 'DROP_LAST': True},
        'OPTIMIZER': {'TYPE': '', 'BASE_LR': 0.001, 'WEIGHT_DECAY': 0.0, 'MAX_GRAD_NORM': 0.0,
                      'SGD': {'momentum': 0.9, 'dampening': 0.0}, 'Adam': {'betas': '(0.9, 0.999)'}},
        'SCHEDULER': {'TYPE': '', 'MAX_ITERATION': 1, 'CLIP_LR': 0.0, 'StepLR': {'step_size': 0, 'gamma': 0.1},
                      'MultiStepLR': {'milestones': '()', 'gamma': 0.1}},
        'TRAIN': {'BATCH_SIZE': 1, 'CHECKPOINT_PERIOD': 0, 'LOG_PERIOD': 0, 'SUMMARY_PERIOD': 0, 'MAX_TO_KEEP': 0,
                  'AUGMENTATION': '()', 'FROZEN_PATTERNS': '()', 'LABEL_WEIGHTS_PATH': ''},
        'VAL': {'BATCH_SIZE': 1, 'PERIOD': 0, 'LOG_PERIOD': 0, 'METRIC': '', 'AUGMENTATION': '()', 'REPEATS': 1},
        'OUTPUT_DIR': '@', 'RNG_SEED': -1,
    })


_PN2SSG = {'num_classes': 20, 'sa_channels': '((32, 32, 64), (64, 64, 128), (128, 128, 256), (256, 256, 512))',
           'num_centroids': '(2048, 512, 128, 32)', 'radius': '(0.1, 0.2, 0.4, 0.8)', 'max_neighbors': '(32, 32, 32, 32)',
           'fp_channels': '((256, 256), (256, 256), (256, 128), (128, 128, 128))', 'fp_neighbors': '(3, 3, 3, 3)',
           'seg_channels': '(128,)', 'dropout_prob': 0.5, 'use_xyz': True}


def get_cfg_mvpnet_3d():
    """mvpnet/config/mvpnet_3d.py:6-80"""
    cfg = _base()
    cfg.merge(CfgNode._convert({
        'TASK': 'mvpnet_3d', 'VAL': {'METRIC': 'seg_iou'},
        'DATASET': {'TRAIN': '', 'VAL': '', 'ScanNet2D3DChunks': {
            'cache_dir': '', 'image_dir': '', 'chunk_size': '(1.5, 1.5)', 'chunk_thresh': 0.3, 'chunk_margin': '(0.2, 0.2)',
            'nb_pts': 8192, 'num_rgbd_frames': 3, 'resize': '(160, 120)', 'k': 3,
            'image_normalizer': '((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))',
            'augmentation': {'z_rot': '()', 'flip': 0.0, 'color_jitter': '()'}}},
        'MODEL_3D': {'TYPE': '', 'PN2SSG': dict(_PN2SSG, in_channels=64)},
        'MODEL_2D': {'TYPE': '', 'CKPT_PATH': '', 'UNetResNet34': {'num_classes': 20, 'p': 0.0}},
        'FEAT_AGGR': {'in_channels': 64, 'mlp_channels': '(64, 64, 64)', 'reduction': 'sum', 'use_relation': True},
    }))
    return cfg


def get_cfg_sem_seg_3d():
    """mvpnet/config/sem_seg_3d.py (PN2SSG baseline: no input feature)"""
    cfg = _base()
    cfg.merge(CfgNode._convert({
        'TASK': 'sem_seg_3d', 'VAL': {'METRIC': 'seg_iou'},
        'DATASET': {'ROOT_DIR': '', 'TRAIN': '', 'VAL': '',
                    'ScanNet3DChunks': {'chunk_size': '(1.5, 1.5)', 'chunk_thresh': 0.3, 'chunk_margin': '(0.2, 0.2)', 'use_color': False},
                    'ScanNet3DScene': {'use_color': False}},
        'MODEL': {'TYPE': '', 'PN2SSG': dict(_PN2SSG, in_channels=0)}}))
    return cfg


def get_cfg_sem_seg_2d():
    """mvpnet/config/sem_seg_2d.py (the 2D stage: UNetResNet34 on single frames, train_2d.py)"""
    cfg = _base()
    cfg.merge(CfgNode._convert({
        'TASK': 'sem_seg_2d', 'VAL': {'METRIC': 'seg_iou'},
        'DATASET': {'ROOT_DIR': '', 'TRAIN': '', 'VAL': '',
                    'ScanNet2D': {'resize': '()', 'normalizer': '((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))',
                                  'augmentation': {'flip': 0.0, 'color_jitter': '()'}}},
        'MODEL': {'TYPE': '', 'UNetResNet34': {'num_classes': 20, 'p': 0.0}}}))
    return cfg


def load_cfg(path=None, text=None, opts=()):
    """Defaults of the YAML's TASK + the YAML + `KEY VALUE` overrides, purged like the reference does."""
    raw = CfgNode()
    if path is not None:
        raw.merge_from_file(path)
    if text is not None:
        raw.merge_from_text(text)
    task = raw.get('TASK', 'mvpnet_3d')
    cfg = {'mvpnet_3d': get_cfg_mvpnet_3d, 'sem_seg_3d': get_cfg_sem_seg_3d, 'sem_seg_2d': get_cfg_sem_seg_2d}[task]()
    cfg.merge(raw)
    cfg.merge_from_list(list(opts))
    purge_cfg(cfg)
    return cfg


def purge_cfg(cfg):
    """common/config/__init__.py:4-17: under a node with TYPE, drop sibling sub-nodes other than cfg[TYPE]."""
    target = cfg.get('TYPE', None)
    for k in [k for k, v in cfg.items() if isinstance(v, CfgNode)]:
        if target is not None and k != target:
            del cfg[k]
        else:
            purge_cfg(cfg[k])


def build_model_sem_seg_3d(cfg):
    """mvpnet/models/build.py:8-20 -> model (loss: mvpnet_amd.mvpnet3d.SegLoss)"""
    from .pn2 import PN2SSG
    assert cfg.TASK == 'sem_seg_3d' and cfg.MODEL.TYPE == 'PN2SSG', (cfg.TASK, cfg.MODEL.TYPE)
    return PN2SSG(**dict(cfg.MODEL.get('PN2SSG', {})))


def build_model_sem_seg_2d(cfg):
    """mvpnet/models/build.py (sem_seg_2d) / mvpnet/models/unet_resnet34.py:127-139 -> model (loss: build_loss_2d)"""
    from .unet_resnet34 import UNetResNet34
    assert cfg.TASK == 'sem_seg_2d' and cfg.MODEL.TYPE == 'UNetResNet34', (cfg.TASK, cfg.MODEL.TYPE)
    return UNetResNet34(**dict(cfg.MODEL.get('UNetResNet34', {})))


def build_loss_2d(cfg):
    """mvpnet/models/unet_resnet34.py:127-139: SegLoss, with the class weights of TRAIN.LABEL_WEIGHTS_PATH (np.loadtxt, float32) when the
    path is non-empty."""
    import numpy as np
    import torch
    from .mvpnet3d import SegLoss
    path = cfg.TRAIN.get('LABEL_WEIGHTS_PATH', '')
    weight = torch.from_numpy(np.loadtxt(path, dtype=np.float32)) if path else None
    if weight is not None and torch.cuda.is_available():
        weight = weight.cuda()  # (as the reference does: the loss then makes no host-to-device copy per step)
    return SegLoss(weight=weight)


def build_batch_2d(cfg, training=True):
    """The 2D config (configs/scannet/unet_resnet34.yaml) as the keyword arguments of scene.sample_train_batch_2d: DATASET.ScanNet2D's
    resize and normalizer; its augmentation (color_jitter, flip) for the training split only (mvpnet/data/build.py passes the
    augmentation to the training split only).  -> dict: resize ((w, h) or None), image_normalizer, color_jitter, flip."""
    assert cfg.TASK == 'sem_seg_2d', cfg.TASK
    if cfg.DATASET.TYPE != 'ScanNet2D':
        raise ValueError('build_batch_2d: DATASET.TYPE {!r} is not the 2D dataset'.format(cfg.DATASET.TYPE))
    node = cfg.DATASET.get('ScanNet2D', {})
    aug = node.get('augmentation', {}) if training else {}
    resize, normalizer, jitter = node.get('resize', ()), node.get('normalizer', ()), aug.get('color_jitter', ())
    return {'resize': tuple(int(v) for v in resize) if resize else None,
            'image_normalizer': tuple(tuple(float(v) for v in part) for part in normalizer) if normalizer else None,
            'color_jitter': tuple(float(v) for v in jitter) if jitter else (), 'flip': float(aug.get('flip', 0.0))}


def build_val(cfg):
    """The YAML's VAL node (common/config/base.py, all three tasks) as what the validation pass takes: batch_size and repeats for
    scene.val_batches (VAL.BATCH_SIZE, VAL.REPEATS: mvpnet/data/build.py:28-47), period -- validate every so many iterations and at the
    last one, 0 = never (train_mvpnet_3d.py:105-106,221) --, metric -- the meter whose global average selects the best checkpoint
    (VAL.METRIC: mvpnet3d.is_better)."""
    val = cfg.VAL
    return {'batch_size': int(val.BATCH_SIZE), 'repeats': int(val.get('REPEATS', 1)), 'period': int(val.PERIOD), 'metric': str(val.METRIC)}


def scannet_label_mapping(tsv_path, labelids_path, ignore_value=-100):
    """The `raw_to_scannet` table of mvpnet/data/scannet_2d.py:86-103 as a (T,) int64 tensor (on the host: move it to the store's device
    once): raw ScanNet id -> nyu40 id (the columns `id` and `nyu40id` of scannetv2-labels.combined.tsv, ids the file does not list -> 0)
    -> the position of that nyu40 id in labelids.txt (20 classes), ignore_value for every other one.  What ops.prepare_labels and
    scene.sample_train_batch_2d take as `mapping` / `label_mapping`."""
    import csv
    import torch
    with open(tsv_path) as f:
        pairs = [(int(row['id']), int(row['nyu40id'])) for row in csv.DictReader(f, delimiter='\t')]
    raw_to_nyu40 = [0] * (max(k for k, _ in pairs) + 1)
    for k, v in pairs:
        raw_to_nyu40[k] = v
    with open(labelids_path) as f:
        class_ids = [int(line.rstrip().split('\t')[0]) for line in f.readlines()]
    assert len(class_ids) == 20, len(class_ids)
    nyu40_to_scannet = [int(ignore_value)] * 41
    for position, class_id in enumerate(class_ids):
        nyu40_to_scannet[class_id] = position
    return torch.tensor([nyu40_to_scannet[v] for v in raw_to_nyu40], dtype=torch.int64)


def build_model_mvpnet_3d(cfg, net_2d=None, load_2d_ckpt=True, freeze_2d=True):
    """mvpnet/models/build.py:23-47.  net_2d=None: built from cfg.MODEL_2D (TYPE UNetResNet34, mvpnet_amd/unet_resnet34.py);
    with freeze_2d (the reference trains MVPNet with the 2D branch frozen, train_mvpnet_3d.py FROZEN_PATTERNS) it gets a folded
    channels-last RUNTIME COPY (unet_resnet34.frozen_inference) while its own parameters keep the reference layout, so full
    MVPNet3D checkpoints of either side load on the other.  MODEL_2D.CKPT_PATH is loaded like the reference does
    (mvpnet_3d.py:78-81) whenever it is non-empty; load_2d_ckpt=False is for synthetic runs without the checkpoint file and
    says so.  A module instance can be supplied instead (e.g. a feature provider); PN2SSG and FeatureAggregation always come
    from cfg."""
    from .pn2 import PN2SSG
    from .mvpnet3d import MVPNet3D
    assert cfg.TASK == 'mvpnet_3d' and cfg.MODEL_3D.TYPE == 'PN2SSG', (cfg.TASK, cfg.MODEL_3D.TYPE)
    built_here = net_2d is None
    if built_here:
        from .unet_resnet34 import UNetResNet34
        assert cfg.MODEL_2D.TYPE == 'UNetResNet34', cfg.MODEL_2D.TYPE
        net_2d = UNetResNet34(**dict(cfg.MODEL_2D.get('UNetResNet34', {})))
    net_3d = PN2SSG(**dict(cfg.MODEL_3D.get('PN2SSG', {})))
    ckpt = cfg.MODEL_2D.get('CKPT_PATH', '')
    if ckpt and not load_2d_ckpt:
        import warnings
        warnings.warn('MODEL_2D.CKPT_PATH ({}) is NOT loaded (load_2d_ckpt=False): the 2D network keeps its random initialisation'.format(ckpt))
    model = MVPNet3D(net_2d, ckpt if load_2d_ckpt else '', net_3d, **dict(cfg.FEAT_AGGR))
    if built_here and freeze_2d:
        net_2d.frozen_inference()
    return model


def build_augmentation(cfg, rng=None):
    """DATASET.ScanNet2D3DChunks.augmentation.{flip, z_rot} of the YAML (mvpnet/data/build.py -> ScanNet2D3DChunks(flip=, z_rot=))
    as the device-side augmentation of mvpnet_amd.augment (None when both are off).  color_jitter: build_color_jitter."""
    from .augment import DeviceAugmentation
    aug = cfg.DATASET.get('ScanNet2D3DChunks', {}).get('augmentation', {})
    flip, z_rot = aug.get('flip', 0.0), aug.get('z_rot', ())
    if not flip and not z_rot:
        return None
    return DeviceAugmentation(flip=flip, z_rot=z_rot, rng=rng)


def build_color_jitter(cfg, training=True):
    """DATASET.ScanNet2D3DChunks.augmentation.color_jitter of the YAML as the tuple scene.sample_train_batch(color_jitter=) and
    augment.draw_color_jitter take; () when it is off, and for validation / test (mvpnet/data/build.py:116-117 passes the augmentation
    to the training split only)."""
    if not training:
        return ()
    jitter = cfg.DATASET.get('ScanNet2D3DChunks', {}).get('augmentation', {}).get('color_jitter', ())
    return tuple(float(v) for v in jitter) if jitter else ()


def build_batch_3d(cfg, training=True):
    """A 3D-baseline config (configs/scannet/3d_baselines/*.yaml) as the keyword arguments of scene.sample_train_batch_3d: DATASET.TYPE and
    its node (mvpnet/data/build.py:45-70) + {TRAIN,VAL}.AUGMENTATION (parse_augmentations, :73-83).  Exactly (("CropPad", n),) with or
    without a bare "RandomRotateZ" behind it is accepted -- the transform lists the four YAMLs use; anything else raises ValueError.
    -> dict: dataset, nb_pts, use_color, z_rot ((-pi, pi), RandomRotateZ's defaults, or None) [, chunk_size, chunk_margin, chunk_thresh]."""
    import math
    assert cfg.TASK == 'sem_seg_3d', cfg.TASK
    dataset = cfg.DATASET.TYPE
    if dataset not in ('ScanNet3DChunks', 'ScanNet3DScene'):
        raise ValueError('build_batch_3d: DATASET.TYPE {!r} is not a 3D-baseline dataset'.format(dataset))
    aug = (cfg.TRAIN if training else cfg.VAL).AUGMENTATION
    aug = tuple(aug) if isinstance(aug, (tuple, list)) else (aug,)
    ok = 1 <= len(aug) <= 2 and isinstance(aug[0], (tuple, list)) and len(aug[0]) == 2 and aug[0][0] == 'CropPad' \
        and isinstance(aug[0][1], int) and not isinstance(aug[0][1], bool) and aug[0][1] >= 1 and (len(aug) == 1 or aug[1] == 'RandomRotateZ')
    if not ok:
        raise ValueError('build_batch_3d: AUGMENTATION must be (("CropPad", n),) or (("CropPad", n), "RandomRotateZ"), not {!r}'.format(aug))
    node = cfg.DATASET.get(dataset, {})
    kwargs = {'dataset': dataset, 'nb_pts': aug[0][1], 'use_color': bool(node.get('use_color', False)),
              'z_rot': (-math.pi, math.pi) if len(aug) == 2 else None}
    if dataset == 'ScanNet3DChunks':
        kwargs.update(chunk_size=tuple(node.get('chunk_size', (1.5, 1.5))), chunk_margin=tuple(node.get('chunk_margin', (0.2, 0.2))),
                      chunk_thresh=node.get('chunk_thresh', 0.3))
    return kwargs


def build_optimizer(cfg, model, capturable=False):
    """common/solver/build.py:7-22.  capturable=True (opt-in): the FusedAdam whose step number and learning rate live on the device, for a
    captured training step (mvpnet3d.GraphedTrainStep(solver='captured')); a ValueError for anything but Adam on float32 GPU parameters."""
    import torch
    name = cfg.OPTIMIZER.TYPE
    if name == '' and not capturable:
        return None
    kwargs = dict(cfg.OPTIMIZER.get(name, {})) if name else {}
    params = [p for p in model.parameters()]
    if capturable:
        if name != 'Adam' or kwargs.get('amsgrad') or 'fused' in kwargs or not params or not all(p.is_cuda and p.dtype == torch.float32 for p in params):
            raise ValueError('build_optimizer(capturable=True) covers OPTIMIZER.TYPE Adam (no amsgrad) on float32 GPU parameters, not {!r}'.format(name))
        from .optim import FusedAdam
        return FusedAdam(params, lr=cfg.OPTIMIZER.BASE_LR, weight_decay=cfg.OPTIMIZER.WEIGHT_DECAY, capturable=True, **kwargs)
    if name == 'Adam' and not kwargs.get('amsgrad') and 'fused' not in kwargs and params and all(p.is_cuda and p.dtype == torch.float32 for p in params):
        from .optim import FusedAdam  # a torch.optim.Adam (same state, same checkpoints) whose step is ONE launch for all parameter tensors
        return FusedAdam(params, lr=cfg.OPTIMIZER.BASE_LR, weight_decay=cfg.OPTIMIZER.WEIGHT_DECAY, **kwargs)
    if name == 'SGD' and not kwargs.get('maximize') and not kwargs.get('differentiable') and 'fused' not in kwargs and 'foreach' not in kwargs \
            and params and all(p.is_cuda and p.dtype == torch.float32 for p in params):
        from .optim import FusedSGD  # a torch.optim.SGD (same state, same checkpoints) whose step is one launch per 124 parameter tensors
        return FusedSGD(params, lr=cfg.OPTIMIZER.BASE_LR, weight_decay=cfg.OPTIMIZER.WEIGHT_DECAY, **kwargs)
    if name in ('Adam', 'AdamW') and 'fused' not in kwargs and params and all(p.is_cuda for p in params):
        kwargs['fused'] = True  # ATen's multi-tensor kernel (three launches for ~80 tensors)
    return getattr(torch.optim, name)(params, lr=cfg.OPTIMIZER.BASE_LR, weight_decay=cfg.OPTIMIZER.WEIGHT_DECAY, **kwargs)


def build_scheduler(cfg, optimizer, capturable=False):
    """common/solver/build.py:25-41 (without ClipLR).  capturable=True (opt-in): optim.DeviceMultiStepLR on a capturable FusedAdam; a
    ValueError for anything but MultiStepLR on such an optimizer."""
    import torch
    name = cfg.SCHEDULER.TYPE
    if capturable:
        from .optim import DeviceMultiStepLR, FusedAdam
        if name != 'MultiStepLR' or not (isinstance(optimizer, FusedAdam) and optimizer.capturable):
            raise ValueError('build_scheduler(capturable=True) covers SCHEDULER.TYPE MultiStepLR on a FusedAdam(capturable=True), not {!r} on {}'.format(
                name, type(optimizer).__name__))
        return DeviceMultiStepLR(optimizer, **dict(cfg.SCHEDULER.get(name, {})))
    if name == '':
        return None
    return getattr(torch.optim.lr_scheduler, name)(optimizer, **dict(cfg.SCHEDULER.get(name, {})))
