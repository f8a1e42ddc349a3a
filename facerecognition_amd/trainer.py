"""The reference's ArcFace training loop on the device (models/arcface/train_arcface.py: EarlyStopping, ArcFaceTrainer).

``ArcFaceTrainer`` keeps the reference's config schema, method names, history and checkpoint schema, and drives the
pieces this package already has: augmentations (``augment.get_train_transforms``), the frozen trunk
(``FRModel.features``), ``ResNet50Layer4``, ``EmbeddingHead``, ``ArcMarginProduct.loss`` and the fused clip + step of
``optim``.  Everything is float32 and bitwise repeatable: the shuffle and the augmentations draw from numpy Generators,
the dropout from a counter, and a checkpoint stores all three, so a resumed run continues bit for bit.  For that
the trainer also puts the engine into its batch-invariant mode (``FR_OPT_BATCH_INVARIANT``; not on fp8 handles), in
which the frozen trunk's bits do not depend on the kernels a handle measured to be fastest or on the batch size.

What differs from the reference, on purpose: the dataloaders that read image files stay out (the trainer takes arrays
of aligned uint8 crops and labels); ``model.freeze_ratio`` must be 0.8 (layer4 + head + class centres train, the
reference's default fine-tune) or 1.0 (head + class centres train on features computed once); ``mixed_precision`` is
accepted and recorded as ``use_amp: False``; TensorBoard and the t-SNE pictures stay out.
"""
from __future__ import annotations

import copy
import json
import time
from pathlib import Path

import numpy as np
import torch
from torch.optim.lr_scheduler import CosineAnnealingLR, ReduceLROnPlateau, StepLR

from . import _native as N
from . import optim as fused_optim
from .arcmargin import ArcMarginProduct, class_accuracy
from .augment import get_train_transforms, get_val_transforms, mixup_data
from .backbone_train import ResNet50Layer4
from .head import EmbeddingHead
from .verification import compute_verification_accuracy

# parameter tensors of torchvision's ResNet-50 without its fc, in ``backbone.parameters()`` order
_BACKBONE_PARAMS = (("conv1 + bn1", 3), ("layer1", 30), ("layer2", 39), ("layer3", 57), ("layer4", 30))


class EarlyStopping:
    """Stops a run whose monitored score has not improved by more than ``min_delta`` for ``patience`` calls in a row.
    mode 'max' watches an accuracy, 'min' a loss.  Attributes as in the reference: ``counter``, ``best_score``,
    ``early_stop``, ``best_epoch``."""

    def __init__(self, patience=10, min_delta=0.001, mode='max', verbose=True):
        self.patience = patience
        self.min_delta = min_delta
        self.mode = mode
        self.verbose = verbose
        self.reset()

    def __call__(self, score, epoch):
        """True when training should stop."""
        if self.best_score is None:
            better = True
        elif self.mode == 'max':
            better = score > self.best_score + self.min_delta
        else:
            better = score < self.best_score - self.min_delta
        if better:
            self.best_score, self.best_epoch, self.counter = score, epoch, 0
            return False
        self.counter += 1
        if self.verbose:
            print(f"EarlyStopping: {self.counter}/{self.patience} (best: {self.best_score:.4f} @ epoch {self.best_epoch + 1})")
        if self.counter >= self.patience:
            self.early_stop = True
            return True
        return False

    def reset(self):
        self.counter = 0
        self.best_score = None
        self.early_stop = False
        self.best_epoch = 0


def load_config(config):
    """The reference's YAML config as a dict (a dict is deep-copied, a path is parsed with ``yaml.safe_load``)."""
    if isinstance(config, dict):
        return copy.deepcopy(config)
    import yaml
    with open(config, "r", encoding="utf-8") as f:
        return yaml.safe_load(f)


def trainable_layers(freeze_ratio: float):
    """What the reference's ``freeze_layers(model, freeze_ratio)`` leaves trainable in the ResNet-50 backbone: the
    names of the stages that hold at least one trainable parameter tensor."""
    total = sum(n for _, n in _BACKBONE_PARAMS)
    first = int(total * freeze_ratio)
    names, start = [], 0
    for name, n in _BACKBONE_PARAMS:
        if first < start + n:
            names.append(name)
        start += n
    return names


def _as_tensor(a):
    return torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a


def _plain(v):
    """Python scalars, lists and dicts only (what json and ``torch.load(weights_only=True)`` accept)."""
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (np.floating,)):
        return float(v)
    return v


class ArcFaceTrainer:
    """config: the reference's schema, a dict or a YAML path.  model: an ``FRModel`` whose trunk stays frozen.
    train / val: ``(images uint8 [N, H, W, 3], labels [N])`` as numpy arrays or tensors.  checkpoint_dir overrides
    ``checkpoint.save_dir``.  seed starts the shuffle, augmentation and dropout streams and the class centres.
    state_dict: the full model under the reference's key names, from which layer4 and the head start and whose trunk
    the checkpoints carry; default ``model.state_dict()``, what the engine was loaded with."""

    def __init__(self, config, model, train, val, checkpoint_dir=None, num_classes=None, seed=0, verbose=True,
                 state_dict=None):
        self.config = load_config(config)
        self.model_engine = model
        self.base_state_dict = dict(model.state_dict() if state_dict is None else state_dict)
        if model.dtype != "fp8":
            # the trunk's bits must not depend on which kernels a handle measured to be fastest, or on the batch size:
            # a resumed run gets another handle and may end an epoch on a smaller batch
            model.set_option(N.FR_OPT_BATCH_INVARIANT, 1)
        self.device = model.device
        self.verbose = verbose
        self.seed = int(seed)
        if checkpoint_dir:
            self.config['checkpoint']['save_dir'] = str(checkpoint_dir)
        self.setup_dirs()
        self.setup_data(train, val, num_classes)
        self.setup_model()
        self.setup_optimizer()
        self.setup_early_stopping()
        self.setup_mixed_precision()
        self.current_epoch = 0
        self.best_val_acc = 0.0
        self.best_val_loss = float('inf')
        self.global_step = 0
        self.grad_norms = []  # device scalars, one per step of the last train_epoch: the gradient norm before clipping
        self.first_grad_norm = None  # that of the very first step
        self.history = {'train_loss': [], 'train_acc': [], 'val_loss': [], 'val_acc': [], 'ver_acc': [],
                        'learning_rate': [], 'epoch': []}

    def _say(self, *a):
        if self.verbose:
            print(*a)

    # -- setup ----------------------------------------------------------------------------------------------------
    def setup_dirs(self):
        self.checkpoint_dir = Path(self.config['checkpoint']['save_dir'])
        self.checkpoint_dir.mkdir(parents=True, exist_ok=True)

    def setup_data(self, train, val, num_classes=None):
        labels = lambda y: (y if isinstance(y, torch.Tensor) else torch.from_numpy(np.asarray(y))).to(torch.int64).cpu()
        self.train_x, self.train_y = _as_tensor(train[0]), labels(train[1])
        self.val_x, self.val_y = _as_tensor(val[0]), labels(val[1])
        for x, y, what in ((self.train_x, self.train_y, "train"), (self.val_x, self.val_y, "val")):
            if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or y.shape != (x.shape[0],):
                raise ValueError(f"ArcFaceTrainer: {what} must be (uint8 images [N, H, W, 3], labels [N])")
        self.num_classes = int(num_classes) if num_classes else int(self.train_y.max()) + 1
        self.batch_size = int(self.config['training']['batch_size'])
        data = self.config.get('data', {})
        self.image_size = int(data.get('image_size', self.model_engine.input_size))
        self.train_transform = get_train_transforms(self.image_size, False, data.get('augment_strength', 'normal'))
        self.val_transform = get_val_transforms(self.image_size, False)
        self.shuffle_rng = np.random.default_rng([self.seed, 0])
        self.augment_rng = np.random.default_rng([self.seed, 1])

    def setup_model(self):
        mc, ac = self.config['model'], self.config['arcface']
        engine = self.model_engine
        ratio = float(mc.get('freeze_ratio', 0.0))
        sd = self.base_state_dict
        if ratio == 0.8:
            if engine.arch != "resnet50_arcface":
                raise ValueError("ArcFaceTrainer: freeze_ratio 0.8 trains backbone.layer4 of resnet50_arcface")
            self.layer4 = ResNet50Layer4.for_model(sd).to(self.device)
        elif ratio == 1.0:
            self.layer4 = None
        else:
            need = [n for n in trainable_layers(ratio) if n != "layer4"]
            raise ValueError(f"ArcFaceTrainer: freeze_ratio {ratio} would train the backbone's {', '.join(need)} as "
                             f"well, which have no training backward here; use 0.8 (layer4 + head + class centres) "
                             f"or 1.0 (head + class centres)")
        self.freeze_ratio = ratio
        self.head = EmbeddingHead.for_arch(engine.arch, sd).to(self.device).seed(self.seed)
        emb = int(mc.get('embedding_size', 512))
        if emb != self.head.embedding_size:
            raise ValueError(f"ArcFaceTrainer: embedding_size {emb} does not match the model's {self.head.embedding_size}")
        self.arcface = ArcMarginProduct(emb, self.num_classes, scale=float(ac['scale']), margin=float(ac['margin']),
                                        easy_margin=bool(ac['easy_margin']))
        with torch.no_grad():  # the centres from a generator of their own, not torch's global stream
            torch.nn.init.xavier_uniform_(self.arcface.weight, generator=torch.Generator().manual_seed(self.seed))
        self.arcface.to(self.device)
        tc = self.config['training']
        self.label_smoothing = float(tc.get('label_smoothing', 0.0))
        mix = tc.get('mixup', {}) or {}
        self.use_mixup = bool(mix.get('enabled', False))
        self.mixup_alpha = float(mix.get('alpha', 0.2))
        if self.use_mixup and self.layer4 is None:
            raise ValueError("ArcFaceTrainer: mixup mixes images; freeze_ratio 1.0 trains on features computed once")
        self._cached = None
        n_train = sum(p.numel() for p in self.trainable_parameters())
        self._say(f"Trainable parameters: {n_train:,} (freeze_ratio {ratio})")

    def modules(self):
        return [m for m in (self.layer4, self.head, self.arcface) if m is not None]

    def trainable_parameters(self):
        return [p for m in self.modules() for p in m.parameters() if p.requires_grad]

    def setup_optimizer(self):
        tc = self.config['training']
        oc = tc['optimizer']
        self.target_lr = oc['lr']
        warm = tc.get('warmup', {}) or {}
        self.warmup_enabled = bool(warm.get('enabled', False))
        self.warmup_epochs = warm.get('epochs', 5)
        self.warmup_start_lr = warm.get('start_lr', 0.0001)
        lr0 = self.warmup_start_lr if self.warmup_enabled else self.target_lr
        clip = tc.get('grad_clip', {}) or {}
        max_norm = float(clip['max_norm']) if clip.get('enabled', False) else None
        kind = oc['type'].lower()
        params = self.trainable_parameters()
        if kind == 'sgd':
            self.optimizer = fused_optim.SGD(params, lr=lr0, momentum=oc['momentum'], weight_decay=oc['weight_decay'],
                                             max_norm=max_norm)
        elif kind == 'adam':
            self.optimizer = fused_optim.Adam(params, lr=lr0, weight_decay=oc.get('weight_decay', 0), max_norm=max_norm)
        elif kind == 'adamw':
            self.optimizer = fused_optim.AdamW(params, lr=lr0, weight_decay=oc.get('weight_decay', 0.01),
                                               max_norm=max_norm)
        else:
            raise ValueError(f"ArcFaceTrainer: optimizer type must be sgd, adam or adamw, not {oc['type']!r}")
        sc = tc['scheduler']
        stype = sc['type'].lower()
        epochs = tc['num_epochs']
        if stype == 'step':
            self.scheduler = StepLR(self.optimizer, step_size=sc['step_size'], gamma=sc['gamma'])
            self.scheduler_type = 'epoch'
        elif stype == 'cosine':
            t_max = epochs - self.warmup_epochs if self.warmup_enabled else epochs
            self.scheduler = CosineAnnealingLR(self.optimizer, T_max=t_max, eta_min=sc.get('eta_min', 1e-6))
            self.scheduler_type = 'epoch'
        elif stype == 'plateau':
            self.scheduler = ReduceLROnPlateau(self.optimizer, mode=sc.get('mode', 'min'), factor=sc.get('factor', 0.1),
                                               patience=sc.get('patience', 5), min_lr=sc.get('min_lr', 1e-7))
            self.scheduler_type = 'metric'
        else:
            self.scheduler = None
            self.scheduler_type = None
        self._say(f"Optimizer: {kind}, target lr {self.target_lr}, scheduler {stype}, clip {max_norm}")

    def setup_early_stopping(self):
        es = self.config['training'].get('early_stopping', {}) or {}
        if es.get('enabled', False):
            self.es_mode = es.get('mode', 'min')
            self.early_stopping = EarlyStopping(patience=es['patience'], min_delta=es.get('min_delta', 0.001),
                                                mode=self.es_mode, verbose=self.verbose)
        else:
            self.early_stopping = None
            self.es_mode = None

    def setup_mixed_precision(self):
        wanted = bool((self.config.get('mixed_precision', {}) or {}).get('enabled', False))
        self.use_amp = False
        self.scaler = None
        self.mixed_precision_message = (
            "mixed_precision.enabled is accepted, but every kernel of this training path is float32: "
            "training runs in float32 and the checkpoint records use_amp: False" if wanted else
            "mixed precision: disabled (float32)")
        self._say(self.mixed_precision_message)

    def get_lr(self):
        return self.optimizer.param_groups[0]['lr']

    # -- forward --------------------------------------------------------------------------------------------------
    def _trunk(self, x):
        with torch.no_grad():
            if self.layer4 is not None:
                return self.model_engine.features(x, at="layer4_in")
            return self.model_engine.features(x)

    def _embed(self, feat):
        return self.head(self.layer4(feat) if self.layer4 is not None else feat)

    def _set_mode(self, train: bool):
        for m in self.modules():
            m.train(train)

    def _batches(self, n, order=None, min_rows=1):
        B = self.batch_size
        for i in range(0, n, B):
            idx = np.arange(i, min(i + B, n)) if order is None else order[i:i + B]
            if len(idx) >= min_rows:
                yield idx

    def train_epoch(self):
        """One epoch over the shuffled training set: (mean loss, accuracy in percent from the pure cosine)."""
        self._set_mode(True)
        n = self.train_x.shape[0]
        order = self.shuffle_rng.permutation(n)
        if self.layer4 is None and self._cached is None:  # features of the un-augmented images, once
            self._cached = torch.cat([self._trunk(self.val_transform(self.train_x[idx].to(self.device), None))
                                      for idx in self._batches(n)])
        running, correct, total, steps = 0.0, 0.0, 0, 0
        self.grad_norms = []
        for idx in self._batches(n, order, min_rows=2):  # batch statistics need two rows
            y = self.train_y[idx].to(self.device)
            yb, lam = None, 1.0
            if self.layer4 is None:
                feat = self._cached[torch.from_numpy(idx).to(self.device)]
            else:
                x = self.train_transform(self.train_x[idx].to(self.device), self.augment_rng)
                if self.use_mixup:
                    x, _, yb, lam = mixup_data(x, y, self.mixup_alpha, generator=self.augment_rng)
                feat = self._trunk(x)
            self.optimizer.zero_grad()
            emb = self._embed(feat)
            loss = self.arcface.loss(emb, y, yb, lam, label_smoothing=self.label_smoothing)
            loss.backward()
            self.optimizer.step()  # clip + update, no host round trip
            self.grad_norms.append(self.optimizer.last_grad_norm)
            if self.first_grad_norm is None:
                self.first_grad_norm = self.grad_norms[0]
            running += float(loss.item())
            correct += class_accuracy(emb.detach(), self.arcface.weight, y) * len(idx)
            total += len(idx)
            steps += 1
            self.global_step += 1
        return running / max(steps, 1), 100.0 * correct / max(total, 1)

    def validate(self):
        """(val loss, classification accuracy %, verification accuracy %, its threshold, embeddings, labels)."""
        self._set_mode(False)
        n = self.val_x.shape[0]
        running, correct, steps, embs = 0.0, 0.0, 0, []
        with torch.no_grad():
            for idx in self._batches(n):
                y = self.val_y[idx].to(self.device)
                emb = self._embed(self._trunk(self.val_transform(self.val_x[idx].to(self.device), None)))
                running += float(self.arcface.loss(emb, y, label_smoothing=self.label_smoothing).item())
                correct += class_accuracy(emb, self.arcface.weight, y) * len(idx)
                embs.append(emb)
                steps += 1
        emb = torch.cat(embs)
        labels = self.val_y.numpy()
        ver_acc, ver_thr, _ = compute_verification_accuracy(emb, labels, num_pairs=min(10000, n * 2))
        return (running / max(steps, 1), 100.0 * correct / max(n, 1), float(ver_acc) * 100.0, float(ver_thr),
                emb.cpu().numpy(), labels)

    # -- checkpoints ----------------------------------------------------------------------------------------------
    def model_state_dict(self):
        """The full model under the reference's key names: the engine's trunk, then the trained layer4, head and
        class centres (CPU tensors).  ``FRModel.load_state_dict`` and the checkpoint loaders take it."""
        sd = {k: torch.as_tensor(np.asarray(v)).clone() if not isinstance(v, torch.Tensor) else v.detach().cpu().clone()
              for k, v in self.base_state_dict.items()}
        if self.layer4 is not None:
            sd.update(self.layer4.reference_state_dict())
        sd.update(self.head.reference_state_dict())
        sd["arcface.weight"] = self.arcface.weight.detach().cpu().clone()
        return sd

    def rng_state(self):
        return {'shuffle': _plain(self.shuffle_rng.bit_generator.state),
                'augment': _plain(self.augment_rng.bit_generator.state),
                'dropout': [int(self.head._seed), int(self.head._offset)]}

    def save_checkpoint(self, val_acc, val_loss, is_best=False):
        ck = {
            'epoch': self.current_epoch,
            'model_state_dict': self.model_state_dict(),
            'optimizer_state_dict': self.optimizer.state_dict(),
            'scheduler_state_dict': self.scheduler.state_dict() if self.scheduler else None,
            'scaler_state_dict': None,
            'val_acc': float(val_acc),
            'val_loss': float(val_loss),
            'best_val_acc': float(self.best_val_acc),
            'best_val_loss': float(self.best_val_loss),
            'config': self.config,
            'num_classes': self.num_classes,
            'global_step': self.global_step,
            'warmup_enabled': self.warmup_enabled,
            'warmup_epochs': self.warmup_epochs,
            'target_lr': self.target_lr,
            'use_amp': self.use_amp,
            'history': self.history,
            'rng_state': self.rng_state(),  # not in the reference: makes a resumed run bitwise
        }
        if is_best:
            torch.save(ck, self.checkpoint_dir / 'arcface_best.pth')
        torch.save(ck, self.checkpoint_dir / 'arcface_last.pth')
        every = self.config['checkpoint'].get('save_interval', 1)
        if (self.current_epoch + 1) % every == 0:
            torch.save(ck, self.checkpoint_dir / f'arcface_epoch_{self.current_epoch + 1}.pth')
            self._cleanup_old_checkpoints()

    def _cleanup_old_checkpoints(self):
        keep = self.config['checkpoint'].get('keep_last_n', 5)
        files = sorted(self.checkpoint_dir.glob('arcface_epoch_*.pth'), key=lambda p: int(p.stem.split('_')[-1]),
                       reverse=True)
        for old in files[keep:]:
            old.unlink()

    def save_training_history(self):
        data = {'history': self.history, 'best_val_acc': self.best_val_acc, 'best_val_loss': self.best_val_loss,
                'total_epochs': self.current_epoch + 1, 'num_classes': self.num_classes,
                'config': {k: self.config.get(k, {}) for k in ('model', 'training', 'arcface')}}
        with open(self.checkpoint_dir / 'training_history.json', 'w', encoding='utf-8') as f:
            json.dump(data, f, indent=2, ensure_ascii=False)

    # -- the loop -------------------------------------------------------------------------------------------------
    def adjust_warmup_lr(self, epoch):
        """Linear warm-up: sets the LR of ``epoch`` and returns True while ``epoch < warmup_epochs``."""
        if not self.warmup_enabled or epoch >= self.warmup_epochs:
            return False
        lr = self.warmup_start_lr + (self.target_lr - self.warmup_start_lr) * ((epoch + 1) / self.warmup_epochs)
        for g in self.optimizer.param_groups:
            g['lr'] = lr
        return True

    def train(self):
        """Epochs ``current_epoch .. num_epochs - 1`` with warm-up, scheduler, checkpoints and early stopping; returns
        the best verification accuracy."""
        t0 = time.time()
        for epoch in range(self.current_epoch, self.config['training']['num_epochs']):
            self.current_epoch = epoch
            warm = self.adjust_warmup_lr(epoch)
            self._say(f"Epoch {epoch + 1}/{self.config['training']['num_epochs']} | LR: {self.get_lr():.2e}"
                      f"{' [WARMUP]' if warm else ''}")
            train_loss, train_acc = self.train_epoch()
            val_loss, val_acc, ver_acc, ver_thr, _, _ = self.validate()
            if self.scheduler and not warm:
                if self.scheduler_type == 'metric':
                    self.scheduler.step(val_loss)
                else:
                    self.scheduler.step()
            self._say(f"Train Loss: {train_loss:.4f} | Train Acc: {train_acc:.2f}% | Val Loss: {val_loss:.4f} | "
                      f"Val Cls Acc: {val_acc:.2f}% | Ver Acc: {ver_acc:.2f}% (threshold={ver_thr:.2f})")
            for key, v in (('epoch', epoch + 1), ('train_loss', train_loss), ('train_acc', train_acc),
                           ('val_loss', val_loss), ('val_acc', val_acc), ('ver_acc', ver_acc),
                           ('learning_rate', float(self.get_lr()))):
                self.history[key].append(v)
            self.save_training_history()
            is_best = ver_acc > self.best_val_acc
            if is_best:
                self.best_val_acc, self.best_val_loss = ver_acc, val_loss
            self.save_checkpoint(ver_acc, val_loss, is_best)
            if self.early_stopping:
                if self.early_stopping(val_loss if self.es_mode == 'min' else ver_acc, epoch):
                    self._say(f"Early stopping; best epoch {self.early_stopping.best_epoch + 1}")
                    break
        self._say(f"Training took {(time.time() - t0) / 3600:.2f} h; best verification accuracy {self.best_val_acc:.2f}%")
        return self.best_val_acc

    def resume_training(self, checkpoint_path, reset_optimizer=False):
        """Continue from a checkpoint of ``save_checkpoint``.  reset_optimizer: keep the fresh optimizer and scheduler
        and take the LR from the config."""
        ck = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        sd = ck['model_state_dict']
        if self.layer4 is not None:
            self.layer4.load_reference_state_dict(sd)
        self.head.load_reference_state_dict(sd)
        with torch.no_grad():
            self.arcface.weight.copy_(sd['arcface.weight'])
        self.model_engine.load_state_dict(sd)
        if reset_optimizer:
            for g in self.optimizer.param_groups:
                g['lr'] = self.config['training']['optimizer']['lr']
        else:
            self.optimizer.load_state_dict(ck['optimizer_state_dict'])
            if ck.get('scheduler_state_dict') and self.scheduler:
                self.scheduler.load_state_dict(ck['scheduler_state_dict'])
        self.current_epoch = ck['epoch'] + 1
        self.best_val_acc = ck['best_val_acc']
        self.best_val_loss = ck.get('best_val_loss', float('inf'))
        self.global_step = ck.get('global_step', 0)
        hist = self.checkpoint_dir / 'training_history.json'
        loaded = False
        if hist.exists():
            try:
                with open(hist, 'r', encoding='utf-8') as f:
                    self.history = json.load(f).get('history', self.history)
                loaded = True
            except (OSError, ValueError) as e:
                self._say(f"Warning: could not read {hist}: {e}")
        if not loaded and 'history' in ck:
            self.history = ck['history']
        if not reset_optimizer and ck.get('warmup_enabled'):
            self.warmup_enabled = ck['warmup_enabled']
            self.warmup_epochs = ck.get('warmup_epochs', 5)
            self.target_lr = ck.get('target_lr', self.config['training']['optimizer']['lr'])
        rng = ck.get('rng_state')
        if rng:
            self.shuffle_rng.bit_generator.state = rng['shuffle']
            self.augment_rng.bit_generator.state = rng['augment']
            self.head.seed(*rng['dropout'])
        self._cached = None
        epochs = self.config['training']['num_epochs']
        if self.current_epoch >= epochs:  # the reference extends a finished run by 50 epochs
            self.config['training']['num_epochs'] = self.current_epoch + 50
        self._say(f"Resumed from epoch {self.current_epoch}, LR {self.get_lr():.2e}, global step {self.global_step}")
