"""``BaseModel`` with the reference's stub surface and checkpoint helpers
(reference ``models/base_model.py:8-131``): same file naming ``<epoch>_net_<label>.pth`` and the same
strict -> subset -> shape-matched fallback when loading."""
import contextlib
import os
from collections import OrderedDict

import torch


class BaseModel(torch.nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.gpu_ids = opt.gpu_ids
        self.isTrain = opt.isTrain
        self.save_dir = os.path.join(opt.checkpoints_dir, opt.name)

    # the reference wraps the training model in DataParallel and the driver talks to ``model.module``;
    # here every rank owns a whole model, so ``module`` is the model itself.
    @property
    def module(self):
        return self

    def name(self):
        return 'BaseModel'

    def set_input(self, input):
        self.input = input

    def forward(self):
        pass

    def test(self):
        pass

    def get_image_paths(self):
        pass

    def optimize_parameters(self):
        pass

    def get_current_visuals(self):
        return self.input

    def get_current_errors(self):
        return {}

    def save(self, label):
        pass

    def _path(self, network_label, epoch_label, save_dir=''):
        return os.path.join(save_dir or self.save_dir, '%s_net_%s.pth' % (epoch_label, network_label))

    def save_network(self, network, network_label, epoch_label, gpu_ids=None):
        os.makedirs(self.save_dir, exist_ok=True)
        sd = {k: v.detach().cpu().clone() for k, v in network.state_dict().items()}
        torch.save(sd, self._path(network_label, epoch_label))

    def save_network_dict(self, network_dict, optimizer, network_label, epoch_label, gpu_ids=None):
        os.makedirs(self.save_dir, exist_ok=True)
        out = {'network': {k: {n: t.detach().cpu().clone() for n, t in v.state_dict().items()}
                           for k, v in network_dict.items()},
               'optimizer': optimizer.state_dict()}
        torch.save(out, self._path(network_label, epoch_label))

    def delete_network(self, network_label, epoch_label, gpu_ids=None):
        p = self._path(network_label, epoch_label)
        if os.path.isfile(p):
            os.remove(p)

    def load_network(self, network, network_label, epoch_label, save_dir=''):
        path = self._path(network_label, epoch_label, save_dir)
        if not os.path.isfile(path):
            print('%s not exists yet!' % path)
            if network_label in ('G', 'G_ema'):
                raise RuntimeError('Generator must exist!')
            return
        self._load_with_fallback(network, torch.load(path, map_location='cpu'), network_label)

    @staticmethod
    def _load_with_fallback(network, loaded, network_label):
        """strict -> the checkpoint's subset of our keys -> shape-matched merge (reference models/base_model.py:76-110)."""
        try:
            network.load_state_dict(loaded)
            return
        except RuntimeError:
            pass
        own = network.state_dict()
        subset = {k: v for k, v in loaded.items() if k in own}
        try:
            network.load_state_dict(subset)
            print('Pretrained network %s has excessive layers; Only loading layers that are used' % network_label)
            return
        except RuntimeError:
            pass
        print('Pretrained network %s has fewer layers; The following are not initialized:' % network_label)
        merged, missing = dict(own), set()
        for k, v in loaded.items():
            if k in own and v.size() == own[k].size():
                merged[k] = v
        for k, v in own.items():
            if k not in loaded or v.size() != loaded[k].size():
                missing.add(k.split('.')[0])
        print(sorted(missing))
        network.load_state_dict(merged)

    def load_network_dict(self, network_dict, optimizer, network_label, epoch_label, save_dir=''):
        path = self._path(network_label, epoch_label, save_dir)
        if not os.path.isfile(path):
            print('%s not exists yet!' % path)
            assert network_label not in ('G', 'G_ema'), 'Generator must exist!'
            return
        ck = torch.load(path, map_location='cpu')
        for k, v in network_dict.items():
            self._load_with_fallback(v, ck['network'][k], '%s.%s' % (network_label, k))
        if optimizer is not None:
            optimizer.load_state_dict(ck['optimizer'])

    def update_learning_rate(self):
        pass

    # ---- gradient guard (--clip_grad_norm F / --skip_nonfinite; off = none of this runs) -------------------------------
    # Both optimizers get optim.FusedAdam.attach_guard: one statistics pass over the gradient arena per step, and an Adam
    # kernel that reads the clip coefficient and the skip flag from device memory.  Nothing here synchronises.
    def _guard_attach(self, opt):
        """Called by a training constructor once the optimizers exist."""
        max_norm = float(getattr(opt, 'clip_grad_norm', 0.0) or 0.0)
        skip = bool(getattr(opt, 'skip_nonfinite', False))
        if max_norm == 0.0 and not skip:
            return
        for o in (getattr(self, 'optimizer_G', None), getattr(self, 'optimizer_D', None)):
            if o is not None:
                o.attach_guard(max_norm, skip)

    def grad_report(self):
        """Gradient norms, clip coefficients and skipped-step counts of the last step, as host floats that merge into the
        dict given to ``Visualizer.print_current_errors`` / ``plot_current_errors``.  It SYNCHRONISES with the device:
        call it at print frequency only.  Without a guard (both options off) it raises."""
        out = {}
        self._ema_join()         # the optimizers may still be running on their own streams
        for tag in ('G', 'D'):
            o = getattr(self, 'optimizer_' + tag, None)
            if o is None or o.guard is None:
                continue
            r = o.grad_report()
            out[tag + '_grad_norm'], out[tag + '_clip_coef'], out[tag + '_skipped'] = r['norm'], r['clip_coef'], r['skipped']
        if not out:
            raise RuntimeError('grad_report(): no gradient guard (train with --clip_grad_norm F or --skip_nonfinite)')
        return out

    # ---- exponential moving average of the generator (--ema_decay; off = none of this runs) ---------------------------
    # The average lives in the generator's FusedAdam (optim.FusedAdam.attach_ema: the Adam kernel updates it in the pass
    # it already makes).  It is a deterministic function of the parameter trajectory: data-parallel ranks each keep their
    # own, identical copy and exchange nothing.  Checkpoint: <epoch>_net_G_ema.pth, the keys / shapes / dtypes of
    # <epoch>_net_G.pth with the parameters averaged and the buffers (BatchNorm statistics, spectral-norm vectors) live;
    # the update count and decay travel in the mapping's ``_metadata`` (as torch's own module versions do), not as keys.
    def _ema_optimizer(self):
        return getattr(self, 'optimizer_G', None)

    def _ema_join(self):
        """Make the current stream own the generator's weights (subclasses join their helper streams)."""
        from ..ops import join_side_stream
        join_side_stream(self.device)

    def _ema_on(self):
        o = self._ema_optimizer()
        return o is not None and o.ema is not None

    def _ema_guard(self):
        o = self._ema_optimizer()
        if o is not None and o._ema_swapped:
            raise RuntimeError('inside ema_weights(): the generator holds its averaged weights, no training step here')

    def _ema_attach(self, opt, pretrained_path='', resume=True):
        """Called by a training constructor once the generator's optimizer exists.  ``resume``: the constructor has loaded
        the generator of --continue_train, so the average is loaded with it."""
        decay = float(getattr(opt, 'ema_decay', 0.0) or 0.0)
        if decay <= 0.0:
            return
        o = self._ema_optimizer()
        o.attach_ema(decay)
        if resume and getattr(opt, 'continue_train', False):
            path = self._path('G_ema', getattr(opt, 'which_epoch', 'latest'), pretrained_path)
            if os.path.isfile(path):
                self._ema_load(torch.load(path, map_location='cpu'))
            else:
                print('%s not found: the weight average starts from the loaded generator' % path)

    def _ema_meta(self, mapping):
        o = self._ema_optimizer()
        out = OrderedDict(mapping)
        out._metadata = OrderedDict(ema=dict(updates=int(o.ema_updates), decay=float(o.ema_decay)))
        return out

    def _ema_read_meta(self, loaded):
        from ..optim import ema_warm_count
        o = self._ema_optimizer()
        meta = (getattr(loaded, '_metadata', None) or {}).get('ema')
        if meta is None:
            print('the EMA checkpoint carries no update count: continuing at the full decay %g' % o.ema_decay)
            o.ema_updates = ema_warm_count(o.ema_decay)
        else:
            o.ema_updates = int(meta['updates'])

    def _ema_save(self, which_epoch):
        """Pix2PixHD layout (one state dict); TwoStreamAE_mask overrides it with its per-module dict."""
        o = self._ema_optimizer()
        os.makedirs(self.save_dir, exist_ok=True)
        torch.save(self._ema_meta(o.ema_state_dict(self.netG)), self._path('G_ema', which_epoch))

    def _ema_load(self, loaded):
        self._ema_optimizer().load_ema_state_dict(self.netG, loaded)
        self._ema_read_meta(loaded)

    @contextlib.contextmanager
    def ema_weights(self):
        """``with model.ema_weights():`` -- the generator's parameters hold their averages inside (swapped in place under
        the live ``nn.Parameter`` views, no third buffer) and the live weights again afterwards, also when the body raises.
        Inference, visuals and the metrics work inside unchanged; a training step raises ``RuntimeError``."""
        from ..ops import invalidate_panels
        o = self._ema_optimizer()
        if not self._ema_on():
            raise RuntimeError('ema_weights(): no weight average (train with --ema_decay > 0)')
        if o._ema_swapped:
            raise RuntimeError('ema_weights() does not nest')
        self._ema_join()
        o.swap_ema()
        invalidate_panels(o.arena.params)        # every cached weight panel is rebuilt from the values now in place
        try:
            yield self
        finally:
            self._ema_join()
            o.swap_ema()
            invalidate_panels(o.arena.params)
