"""Fused Adam for the networks built from this package.

All parameters live in one flat float32 buffer (each `p.data` becomes a view of it, each `p.grad` a view of one flat
gradient buffer), so that an optimizer step is one elementwise HIP kernel (csrc/fc_optim.hip through fc_adam_step) and
`zero_grad` at most one fill.  The step counter lives on the device: the update is capturable in a HIP graph together with the
forward and backward passes (fieldconv_amd.utils.StepGraph).  Arithmetic of torch.optim.Adam (L2 weight decay, no amsgrad).

Controls (keyword arguments; with every one at its default step() is the two launches above, bit for bit).  Any of them moves the
step to fc_adam_step_ctl: three launches, no atomics, no host synchronisation, everything it needs allocated by the constructor.

    device_lr               the learning rate lives in the (1,) device tensor `opt.lr`, which the kernel reads: a captured step
                            follows `opt.set_lr(...)` between replays.  (Every other control implies it.)
    max_grad_norm           global-norm clipping with torch's clip_grad_norm_ formula.  The gradient is scaled INSIDE the update:
                            `.grad` keeps the unclipped values (clip_grad_norm_ rewrites them).
    skip_nonfinite          a step whose flat gradient holds a NaN or an infinity changes nothing: parameters, moments, EMA and the
                            step count keep their bits, and `opt.stats` counts it.
    decoupled_weight_decay  AdamW: p *= 1 - lr * weight_decay before the update, no L2 term in the gradient.
    ema_decay               an exponential moving average of the parameters, updated in the same kernel:
                            `opt.ema_parameters()`, `with opt.swap_ema():`.
"""
import contextlib

import torch

from . import _lib
from ._launch import _p, _po, on as _on, scratch as _scratch, stream as _stream


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, *, decoupled_weight_decay=False,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None, device_lr=False):
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError(f'FusedAdam: max_grad_norm must be positive (None: no clipping), got {max_grad_norm!r}')
        if ema_decay is not None and not 0 <= float(ema_decay) < 1:
            raise ValueError(f'FusedAdam: ema_decay must lie in [0, 1) (None: no moving average), got {ema_decay!r}')
        params = [p for p in params]
        if not params:
            raise ValueError('FusedAdam needs at least one parameter')
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) != 1:
            raise ValueError('FusedAdam keeps one flat buffer: one parameter group')
        ps = self.param_groups[0]['params']
        dev = ps[0].device
        for p in ps:
            if p.dtype != torch.float32 or p.device != dev or not p.is_cuda:
                raise ValueError('FusedAdam: float32 parameters on one ROCm device (complex filters are stored as real pairs '
                                 'by the modules of this package)')
        sizes = [p.numel() for p in ps]
        offs, total = [], 0
        for n in sizes:                     # every tensor starts on a 16-byte boundary
            offs.append(total)
            total += (n + 3) // 4 * 4
        self._n = total
        self._flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self._grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self._m = torch.zeros(total, dtype=torch.float32, device=dev)
        self._v = torch.zeros(total, dtype=torch.float32, device=dev)
        self._step = torch.zeros(1, dtype=torch.float32, device=dev)
        self._offsets, self._sizes = offs, sizes
        self._views = []                    # the gradient views, one per parameter
        with torch.no_grad():
            for p, o, n in zip(ps, offs, sizes):
                view = self._flat[o:o + n].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p.grad = self._grad[o:o + n].view(p.shape)
                self._views.append(p.grad)
        # The padding entries of the flat gradient buffer start at zero and no view reaches them (every write to the buffer goes
        # through a view), so they stay zero and the global norm is the norm of the gradients alone.
        base = self._grad.data_ptr()
        assert all(v.data_ptr() == base + 4 * o and v.numel() == n and o % 4 == 0 and o + n <= nxt
                   for v, o, n, nxt in zip(self._views, offs, sizes, offs[1:] + [total]))
        # ---- the controls: everything fc_adam_step_ctl needs is allocated here, nothing in step()
        self.decoupled_weight_decay, self.skip_nonfinite = bool(decoupled_weight_decay), bool(skip_nonfinite)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self._ctl = bool(device_lr) or self.decoupled_weight_decay or self.skip_nonfinite or self.max_grad_norm is not None \
            or self.ema_decay is not None
        self.lr = self.stats = self._ema = self._swap = self._ws = None
        if self._ctl:
            self.lr = torch.full((1,), float(lr), dtype=torch.float32, device=dev)
            self._lr_pushed = lr            # the value of param_groups[0]['lr'] that self.lr answers to
            self.stats = torch.zeros(4, dtype=torch.float32, device=dev)
            self._ws = _scratch(_lib.load().fc_adam_ctl_workspace_bytes(total), dev)
            if self.ema_decay is not None:
                self._ema = self._flat.clone()
                self._swap = torch.empty_like(self._flat)
        self._built = True

    def add_param_group(self, param_group):
        if getattr(self, '_built', False):
            raise RuntimeError('FusedAdam keeps every parameter in one flat buffer laid out at construction: '
                               'parameter groups cannot be added afterwards')
        super().add_param_group(param_group)

    # ---- the controls' interface -------------------------------------------------------------------------------------------------
    def _need(self, what, have):
        if not have:
            raise RuntimeError(f'FusedAdam.{what}: this optimizer was built without the control it belongs to')

    @torch.no_grad()
    def set_lr(self, value):
        """Write the device learning rate; no synchronisation.  A float is filled in (and becomes param_groups[0]['lr']); a (1,)
        device tensor is copied, and then param_groups[0]['lr'] is stale until it is assigned again.  The interface between the
        replays of a captured step, where step() itself never writes the rate."""
        self._need('set_lr', self._ctl)
        g = self.param_groups[0]
        if isinstance(value, torch.Tensor):
            self.lr.copy_(value.reshape(1))
        else:
            g['lr'] = value
            self.lr.fill_(float(value))
        self._lr_pushed = g['lr']

    def grad_norm(self):
        """0-dim view of opt.stats: the global gradient norm of the last step, before clipping (0 unless max_grad_norm or
        skip_nonfinite is set).  No synchronisation."""
        self._need('grad_norm', self._ctl)
        return self.stats[0]

    def skipped(self):
        """(2,) view of opt.stats: [1 if the last step was skipped else 0, number of steps skipped so far].  No synchronisation."""
        self._need('skipped', self._ctl)
        return self.stats[2:]

    def ema_parameters(self):
        """views of the moving average, shaped like the parameters and in their order"""
        self._need('ema_parameters', self._ema is not None)
        return [self._ema[o:o + n].view(p.shape) for p, o, n in zip(self.param_groups[0]['params'], self._offsets, self._sizes)]

    @contextlib.contextmanager
    def swap_ema(self):
        """`with opt.swap_ema():` -- the parameters hold the moving average inside the block and their live values, bit for bit,
        after it: three flat copies through a scratch buffer of the constructor's.  Not inside a capture, and no step() inside."""
        self._need('swap_ema', self._ema is not None)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('FusedAdam.swap_ema: not while a graph is being captured (the swap would be replayed with every step)')
        with torch.no_grad():
            self._swap.copy_(self._flat)
            self._flat.copy_(self._ema)
        try:
            yield self
        finally:
            with torch.no_grad():
                self._flat.copy_(self._swap)

    def state_dict(self):
        """torch.optim.Adam's layout: per-parameter `step`, `exp_avg`, `exp_avg_sq` (copies of the flat buffers' slices),
        so that a checkpoint written here resumes under torch.optim.Adam and vice versa -- exactly when every parameter got a
        gradient in every step (see _pack_grads); every entry carries the shared step count.  With ema_decay every entry also
        carries `ema`; with any control the group carries `n_skipped`."""
        ps = self.param_groups[0]['params']
        step = self._step.detach().clone().reshape(())
        state = {i: {'step': step.clone(), 'exp_avg': self._m[o:o + n].view(p.shape).clone(),
                     'exp_avg_sq': self._v[o:o + n].view(p.shape).clone()}
                 for i, (p, o, n) in enumerate(zip(ps, self._offsets, self._sizes))}
        if self._ema is not None:
            for i, e in enumerate(self.ema_parameters()):
                state[i]['ema'] = e.clone()
        group = {k: v for k, v in self.param_groups[0].items() if k != 'params'}
        group['params'] = list(range(len(ps)))
        if self._ctl:
            group['n_skipped'] = int(self.stats[3].item())
        return {'state': state, 'param_groups': [group]}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        groups = state_dict['param_groups']
        ps = self.param_groups[0]['params']
        if len(groups) != 1 or len(groups[0]['params']) != len(ps):
            raise ValueError('FusedAdam.load_state_dict: expected one parameter group with '
                             f'{len(ps)} parameters')
        for k, v in groups[0].items():
            if k != 'params' and k in self.param_groups[0]:
                self.param_groups[0][k] = v
        state = state_dict['state']
        steps = set()
        for i, (p, o, n) in enumerate(zip(ps, self._offsets, self._sizes)):
            st = state.get(i, state.get(str(i)))
            if self._ema is not None:           # a checkpoint without `ema` (plain Adam's): the average starts from the parameters
                self._ema[o:o + n].copy_((st['ema'] if st is not None and 'ema' in st else p.data).reshape(-1))
            if st is None:                      # a parameter that never received a gradient under torch.optim.Adam
                self._m[o:o + n].zero_()
                self._v[o:o + n].zero_()
                continue
            self._m[o:o + n].copy_(st['exp_avg'].reshape(-1))
            self._v[o:o + n].copy_(st['exp_avg_sq'].reshape(-1))
            steps.add(float(st['step']))
        if len(steps) > 1:
            raise ValueError('FusedAdam keeps one step counter: the checkpoint has parameters at different steps')
        self._step.fill_(steps.pop() if steps else 0.0)
        if self._ctl:
            self.set_lr(self.param_groups[0]['lr'])
            self.stats.zero_()
            self.stats[3] = float(groups[0].get('n_skipped', 0))

    def zero_grad(self, set_to_none=True):
        """set_to_none=True (the default, as in torch.optim): the parameters are detached from the flat buffer, autograd assigns
        every gradient, and step() packs them with one multi-tensor copy -- no fill and no add kernel per parameter tensor
        (the segmentation network's training step: 2.99 -> 2.54 ms eager, 1.81 -> 1.71 ms as one HIP graph).
        set_to_none=False: one fill, the gradient views stay in place and backward accumulates into them."""
        if set_to_none:
            for p in self.param_groups[0]['params']:
                p.grad = None
        else:
            self._grad.zero_()

    def _pack_grads(self):
        """Gradients that autograd assigned (after zero_grad(set_to_none=True)) go into the flat buffer; .grad points into the
        buffer again.  A parameter WITHOUT a gradient counts as having a zero gradient: the one elementwise kernel updates the
        whole flat buffer with one shared step counter, so its moments decay and weight decay applies, where torch.optim.Adam
        would skip it (and keep a per-parameter step).  The two agree whenever every parameter handed to the optimizer receives
        a gradient every step -- true for the networks of this package (the `phase` of ftype 0 / 2 layers is a buffer, not a
        parameter); frozen or unused parameters should not be given to FusedAdam."""
        lo, hi = self._grad.data_ptr(), self._grad.data_ptr() + 4 * self._n
        views, grads = [], []
        for p, v in zip(self.param_groups[0]['params'], self._views):
            gr = p.grad
            if gr is None:
                v.zero_()
            elif not (lo <= gr.data_ptr() < hi):
                if gr.shape != v.shape or gr.dtype != v.dtype or gr.device != v.device:
                    raise RuntimeError('FusedAdam: a parameter\'s .grad does not match the parameter')
                views.append(v)
                grads.append(gr)
            else:
                continue
            p.grad = v
        if views:
            torch._foreach_copy_(views, grads)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        g = self.param_groups[0]
        self._pack_grads()
        lib = _lib.load()
        if self._ctl:
            return self._step_ctl(lib, g, loss)
        with _on(self._flat.device):
            _lib.check(lib.fc_adam_step(_p(self._flat), _p(self._grad), _p(self._m), _p(self._v), _p(self._step), self._n, float(g['lr']),
                                        float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay']), _stream()),
                       'fc_adam_step')
        return loss

    def _step_ctl(self, lib, g, loss):
        """fc_adam_step_ctl.  Eager: a param_groups[0]['lr'] that moved since the last push (a torch.optim.lr_scheduler) is pushed
        first.  While the stream is capturing nothing writes the rate -- a captured fill would reset it on every replay -- and
        set_lr between replays is the interface.  betas, eps, weight_decay and the controls are constants of a captured step."""
        with _on(self._flat.device):
            if g['lr'] != self._lr_pushed and not torch.cuda.is_current_stream_capturing():
                self.set_lr(g['lr'])
            ctl = _lib.FcAdamCtl(float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay']),
                                 int(self.decoupled_weight_decay), self.max_grad_norm or 0.0, int(self.skip_nonfinite),
                                 -1.0 if self.ema_decay is None else self.ema_decay)
            _lib.check(lib.fc_adam_step_ctl(_p(self._flat), _p(self._grad), _p(self._m), _p(self._v), _po(self._ema), _p(self._step),
                                            _p(self.lr), _p(self.stats), _p(self._ws), self._ws.numel(), self._n, ctl, _stream()),
                       'fc_adam_step_ctl')
        return loss
