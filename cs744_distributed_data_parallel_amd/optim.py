"""Fused SGD (momentum, dampening, weight decay, Nesterov, maximize) over flat arenas.

Drop-in for ``torch.optim.SGD`` as used by every reference stage
(``optim.SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=0.0001)``,
``/root/reference/src/Part 1/main.py:114-115``): it *is* a ``torch.optim.Optimizer`` subclass, so
``param_groups``, ``state_dict()`` / ``load_state_dict()`` (``momentum_buffer`` per parameter) and
LR schedulers behave exactly like torch's.

MI355X path: parameters, gradients and momentum live in :class:`~.utils.arena.FlatArena` storages,
so a param group whose parameters form one contiguous arena run is updated by ONE vectorised HIP
kernel (float4, fma order matching ATen's ``add(alpha=...)``) instead of one launch per tensor.
``zero_grad`` zeroes the gradient arena in place (the arena views stay attached, which keeps the
bucketed reducer zero-copy). The learning rate can live on the device (``lr_tensor``) so a captured
hipGraph step follows an LR schedule without re-capture.

Gradient clipping (``max_grad_norm``) and non-finite step skipping (``skip_nonfinite``) ride in the
same launch: one extra dispatch writes fp64 partial sums of squares of the gradient arena, and every
workgroup of the SGD kernel derives the global norm and ``coef = min(max_grad_norm / (norm + 1e-6), 1)``
from them in its prologue -- no second pass over the gradients, no host sync, so a captured step
clips with the norm of each replay. Unlike ``torch.nn.utils.clip_grad_norm_``, the fused path leaves
``p.grad`` UNSCALED (the coefficient is applied as the kernel reads the gradient); the reference
paths (CPU, ``force_reference``, per-parameter launches) scale it in place as torch does. With
``skip_nonfinite`` a step whose norm is inf / NaN leaves parameters and momentum bitwise unchanged
(counted in ``skipped_steps``); :func:`clip_grad_norm_` is the stand-alone, in-place form.

:class:`LARS` is the same step with a per-parameter trust ratio (layer-wise adaptive rate scaling, for
large global batches), derived on the device in the same way from per-parameter sums of squares.

Weight EMA (``ema_decay``): ``e <- d * e + (1 - d) * w`` after every step, in the same launch again: the
updated weight is in registers, ``e`` (a fourth arena storage, ``state[p]["ema_buffer"]``) is one more
load and store. ``d`` and ``1 - d`` live on the device (``set_ema_decay``), so a captured step follows
a decay warm-up without re-capture. A step skipped by ``skip_nonfinite`` leaves ``e`` unchanged, as
does a step for a parameter without a gradient. ``ema_weights()`` swaps ``e`` into the model for
evaluation; BatchNorm running statistics are not averaged (they are a moving average already).

Learning-rate schedule (``lr_schedule``, an :class:`LRSchedule`): the rate of step ``t`` is
``float32(base * f(t))`` with ``f`` a warm-up into a constant, cosine, polynomial or multi-step phase and
``base`` what the step would use otherwise (``param_groups[i]["lr"]`` / ``lr_tensor``). The fused kernels
evaluate ``f`` themselves in their prologue from a device step counter and advance that counter in the
same launch (an arrival count over the workgroups), so the schedule costs no launch, needs no host value
and a captured step changes its own rate at every replay. ``schedule_step``, ``last_lr``,
``set_schedule_step``, ``set_lr_schedule`` and ``lr_schedule_table`` are the handles; ``state_dict()``
carries the step as ``param_groups[i]["lr_schedule_step"]``. One schedule for all param groups; a step
skipped by ``skip_nonfinite`` still counts (the schedule counts iterations).

:class:`AdamW` and :class:`LAMB` are the Adam family over the same arenas, with the same options under the
same names: ``exp_avg`` in the momentum storage, ``exp_avg_sq`` in a second one beside it, the step count of
the bias corrections in a device word that the fused kernel (``csrc/kernels/adam.hip``) reads and advances
itself. They do not emit the next forward's weight preparation; see the classes.
"""
from __future__ import annotations

import contextlib
import math

import torch
from torch.optim import Optimizer

from . import _native
from .utils.arena import _view_like, arena_for


_LR_KINDS = {"constant": 0, "cosine": 1, "poly": 2, "step": 3}
_LR_MAX_MILESTONES = 8


class LRSchedule:
    """A learning-rate factor ``f(t)`` of the step index ``t >= 0`` (the number of ``step()`` calls so far),
    for ``SGD(..., lr_schedule=...)`` / ``LARS(..., lr_schedule=...)``:

    * ``t < warmup_steps``: ``f = s + (1 - s) * t / warmup_steps``, ``s = warmup_start_factor`` (linear
      warm-up, Goyal et al.);
    * afterwards, with ``u = (t - warmup_steps) / (total_steps - warmup_steps)``:
      ``constant``: 1; ``cosine``: ``r + (1 - r) * (1 + cos(pi u)) / 2``; ``poly``: ``r + (1 - r) * (1 - u) ** power``
      (1: linear decay, 2: the LARS paper's); both are ``r = end_factor`` itself from ``total_steps`` on;
      ``step``: ``gamma ** k``, ``k`` the number of ``milestones <= t``.

    Everything is evaluated in fp64; :meth:`factor` is the formula in Python floats (what the CPU and
    reference paths use), the fused kernels evaluate the same one on the device. The defaults are the
    conventional ones; nothing was measured to choose them."""

    def __init__(self, kind: str = "cosine", total_steps: int | None = None, warmup_steps: int = 0,
                 warmup_start_factor: float = 0.0, end_factor: float = 0.0, power: float = 2.0,
                 milestones=(), gamma: float = 0.1):
        if kind not in _LR_KINDS:
            raise ValueError(f"Invalid lr schedule kind: {kind!r} (one of {', '.join(_LR_KINDS)})")
        if int(warmup_steps) != warmup_steps or warmup_steps < 0:
            raise ValueError(f"Invalid warmup_steps: {warmup_steps}")
        s = float(warmup_start_factor)
        if math.isnan(s) or not 0.0 <= s <= 1.0:
            raise ValueError(f"Invalid warmup_start_factor: {warmup_start_factor}")
        if kind in ("cosine", "poly"):
            if total_steps is None or int(total_steps) != total_steps or not total_steps > warmup_steps:
                raise ValueError(f"Invalid total_steps: {total_steps} ({kind} needs total_steps > warmup_steps)")
        elif total_steps is not None and (int(total_steps) != total_steps or total_steps < 0):
            raise ValueError(f"Invalid total_steps: {total_steps}")
        if not float(end_factor) >= 0.0 or math.isinf(float(end_factor)):
            raise ValueError(f"Invalid end_factor: {end_factor}")
        if not float(power) > 0.0 or math.isinf(float(power)):
            raise ValueError(f"Invalid power: {power}")
        if not float(gamma) > 0.0 or math.isinf(float(gamma)):
            raise ValueError(f"Invalid gamma: {gamma}")
        ms = list(milestones)
        if len(ms) > _LR_MAX_MILESTONES:
            raise ValueError(f"Invalid milestones: at most {_LR_MAX_MILESTONES}, got {len(ms)}")
        if any(int(m) != m or m < 0 for m in ms) or any(b <= a for a, b in zip(ms, ms[1:])):
            raise ValueError(f"Invalid milestones: {milestones} (non-negative integers, strictly increasing)")
        self.kind = kind
        self.total_steps = int(total_steps) if total_steps is not None else 0
        self.warmup_steps = int(warmup_steps)
        self.warmup_start_factor = s
        self.end_factor = float(end_factor)
        self.power = float(power)
        self.milestones = tuple(int(m) for m in ms)
        self.gamma = float(gamma)

    def factor(self, t: int) -> float:
        t = int(t)
        if t < 0:
            raise ValueError(f"Invalid step index: {t}")
        W, T = self.warmup_steps, self.total_steps
        if t < W:
            s = self.warmup_start_factor
            return s + (1.0 - s) * t / W
        if self.kind in ("cosine", "poly"):
            r = self.end_factor
            if t >= T:
                return r
            u = (t - W) / (T - W)
            if self.kind == "cosine":
                return r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * u))
            return r + (1.0 - r) * math.pow(1.0 - u, self.power)
        if self.kind == "step":
            f = 1.0
            for m in self.milestones:
                if m <= t:
                    f *= self.gamma
            return f
        return 1.0

    def rate(self, base: float, t: int) -> float:
        """``float32(base * factor(t))`` as a Python float: the rate of step ``t``."""
        return torch.tensor(float(base) * self.factor(t), dtype=torch.float64).to(torch.float32).item()

    def _pack_args(self):
        return (_LR_KINDS[self.kind], self.warmup_steps, self.warmup_start_factor, self.total_steps, self.end_factor,
                self.power, list(self.milestones), self.gamma)

    def __repr__(self):
        return (f"LRSchedule(kind={self.kind!r}, total_steps={self.total_steps}, warmup_steps={self.warmup_steps}, "
                f"warmup_start_factor={self.warmup_start_factor}, end_factor={self.end_factor}, power={self.power}, "
                f"milestones={self.milestones}, gamma={self.gamma})")


class SGD(Optimizer):
    def __init__(
        self,
        params,
        lr: float = 1e-3,
        momentum: float = 0.0,
        dampening: float = 0.0,
        weight_decay: float = 0.0,
        nesterov: bool = False,
        *,
        maximize: bool = False,
        flat: bool = True,
        max_grad_norm: float | None = None,
        skip_nonfinite: bool = False,
        ema_decay: float | None = None,
        lr_schedule: LRSchedule | None = None,
    ):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self._check_common(max_grad_norm, ema_decay, lr_schedule)
        defaults = dict(
            lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
            maximize=maximize, foreach=None, differentiable=False, fused=None,
        )
        defaults.update(getattr(self, "_extra_defaults", {}))  # a subclass's own param_group entries (LARS)
        super().__init__(params, defaults)
        self._init_common(flat, max_grad_norm, skip_nonfinite, ema_decay, lr_schedule)

    @staticmethod
    def _check_common(max_grad_norm, ema_decay, lr_schedule):
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        if ema_decay is not None:
            _check_ema_decay(ema_decay)
        if lr_schedule is not None and not isinstance(lr_schedule, LRSchedule):
            raise TypeError(f"lr_schedule must be an LRSchedule, not {type(lr_schedule).__name__}")

    def _init_common(self, flat, max_grad_norm, skip_nonfinite, ema_decay, lr_schedule):
        """What every optimizer of the family sets up after ``Optimizer.__init__``: the arena, the clip's,
        the EMA's and the schedule's device words (SGD / LARS here, AdamW / LAMB below)."""
        # callables run at the end of every step (DistributedDataParallel.early_buffer_broadcast
        # joins its end-of-backward buffer broadcast here, after the SGD it overlaps)
        self._post_step_joins = []
        self._flat = flat
        self._arena = None
        self._lr_tensor = None
        self._steps = 0
        self.fused_prep = True  # emit the next step's weight preparation from the step (one arena pass)
        self._step_counter = None  # a device step counter this step advances (DeviceLoader.advance_with)
        self._counter_pending = None
        self._overlap = None  # this iteration's per-bucket steps, run by a DDP reducer (bucket_steps)
        all_params = [p for g in self.param_groups for p in g["params"]]
        if flat and all_params and all_params[0].is_cuda:
            self._arena = arena_for(all_params)
            self._arena.on_relayout(self._on_relayout)
        # gradient-norm clipping / non-finite step skipping: optimizer attributes, not param_group
        # entries, so state_dict() stays torch's
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._clip_part = self._clip_stats = None
        self._clip_fused = False
        if self.skip_nonfinite and any(g.get("dampening", 0) != 0 for g in self.param_groups):
            # a skipped first momentum step zeroes the buffer and the next computes
            # buf = (1 - dampening) * d_p: torch's first-step buf = d_p only for dampening 0
            raise ValueError("skip_nonfinite requires zero dampening")
        if self._clip_enabled and all_params:
            # allocated here, never inside a capture: the partial sums of squares of the norm kernel
            # and {norm, coef, skipped steps} (device-side; grad_norm / clip_coef / skipped_steps)
            dev = all_params[0].device
            self._clip_stats = torch.zeros(4, dtype=torch.float32, device=dev)
            if dev.type == "cuda":
                self._clip_part = torch.zeros(1024, dtype=torch.float64, device=dev)
        # weight EMA: an optimizer attribute like the clip options; None allocates nothing
        self._ema_decay = None
        self._ema_d = self._ema_omd = 0.0  # float32(d), float32(1 - d) as Python floats
        self._ema_coef = None  # {d, 1 - d} on the device, read by the fused kernels' prologue
        if ema_decay is not None and all_params:
            dev = all_params[0].device
            if dev.type == "cuda":
                self._ema_coef = torch.zeros(2, dtype=torch.float32, device=dev)  # never inside a capture
            self._ema_decay = float(ema_decay)
            self.set_ema_decay(ema_decay)
            self.reset_ema()
        # learning-rate schedule: an optimizer attribute again; None allocates nothing
        self._lr_schedule = None
        self._sched_state = self._sched_last = self._sched_cfg = None
        self._sched_pending = False  # this step()'s advance of t, until a launch (or the fallback) takes it
        self._sched_take = False  # whether the group being stepped holds the step()'s last launch
        self._sched_gi = 0  # the group being stepped
        self._sched_host = None  # (t, factor) of this step() where a reference path asked for the rate
        if lr_schedule is not None and all_params:
            dev = all_params[0].device
            # allocated here, never inside a capture: {t, arrivals}, the rate of the last step and, on the
            # GPU, the configuration the kernels read
            self._sched_state = torch.zeros(2, dtype=torch.int64, device=dev)
            self._sched_last = torch.zeros(1, dtype=torch.float32, device=dev)
            if dev.type == "cuda" and _native.available():
                self._sched_cfg = torch.zeros(128, dtype=torch.uint8, device=dev)
            self._lr_schedule = lr_schedule
            self.set_lr_schedule(lr_schedule)

    # ------------------------------------------------------------------ gradient clipping
    @property
    def _clip_enabled(self) -> bool:
        return self.max_grad_norm is not None or self.skip_nonfinite

    @property
    def grad_norm(self):
        """Global gradient 2-norm of the last step: a 0-dim device view (reading it here never syncs);
        None unless ``max_grad_norm`` / ``skip_nonfinite`` is set."""
        return self._clip_stats[0] if self._clip_stats is not None else None

    @property
    def clip_coef(self):
        """``min(max_grad_norm / (grad_norm + 1e-6), 1)`` of the last step (0-dim device view)."""
        return self._clip_stats[1] if self._clip_stats is not None else None

    @property
    def skipped_steps(self):
        """Steps skipped for an inf / NaN gradient norm so far (0-dim device view, a float count)."""
        return self._clip_stats[2] if self._clip_stats is not None else None

    def _clip_fusable(self) -> bool:
        """Whether the clip can ride in this step's flat launch (see :meth:`_flat_fusable`)."""
        return self._clip_part is not None and self._flat_fusable()

    def _flat_fusable(self) -> bool:
        """Whether this step runs as one flat launch (or the split plan's launches) over one arena
        range, so a whole-model quantity can ride in it: one param group, all of its parameters with
        gradients, one contiguous arena run, momentum buffers all first or all later."""
        if self._arena is None or len(self.param_groups) != 1 or _native.force_reference():
            return False
        group = self.param_groups[0]
        params = group["params"]
        if not params or any(p.grad is None or not p.is_cuda for p in params):
            return False
        if self._arena.contiguous_range(params) is None:
            return False
        if any(getattr(p, "_cdp_arena", None) is not self._arena for p in params):
            return False
        if group.get("momentum", 0.0) != 0.0:  # (the Adam family has no first-step rule)
            firsts = self._first_flags(params)
            if any(firsts) and not all(firsts):
                return False
        return True

    def _clip_reference(self, params) -> bool:
        """The clip outside the fused launch (CPU, ``force_reference``, per-parameter launches):
        total norm and coefficient with torch ops exactly as ``torch.nn.utils.clip_grad_norm_``
        computes them, gradients scaled in place as it does. Returns True when the step is to be
        skipped (``skip_nonfinite`` and an inf / NaN norm; a host read)."""
        grads = [p.grad for p in params]
        norms = [torch.linalg.vector_norm(g, 2.0) for g in grads]
        total = torch.linalg.vector_norm(torch.stack([n.to(norms[0].device) for n in norms]), 2.0)
        st = self._clip_stats
        st[0].copy_(total)
        if self.skip_nonfinite and not bool(torch.isfinite(total)):
            st[1].fill_(float("nan") if self.max_grad_norm is not None else 1.0)
            st[2] += 1
            return True
        if self.max_grad_norm is None:
            st[1].fill_(1.0)
            return False
        coef = torch.clamp(self.max_grad_norm / (total + 1e-6), max=1.0)
        st[1].copy_(coef)
        for g in grads:
            g.mul_(coef.to(g.device))
        return False

    def _on_relayout(self, arena):
        # the arena moved the momentum / EMA values with their parameters; re-point the state views
        if arena.momentum is not None:
            views = arena.momentum_views()
            for p in arena.params:
                st = self.state.get(p)
                if st and st.get("momentum_buffer") is not None:
                    st["momentum_buffer"] = views[p._cdp_index]
        if self._ema_decay is not None and arena is self._arena and arena.ema is not None:
            views = arena.ema_views()
            for p in arena.params:
                st = self.state.get(p)
                if st and st.get("ema_buffer") is not None:
                    st["ema_buffer"] = views[p._cdp_index]

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._adopt_momentum()
        self._adopt_ema()
        # the schedule's step: applied when the state carries it, t left alone when it does not; never a
        # live param_groups entry
        ts = [g.pop("lr_schedule_step") for g in self.param_groups if "lr_schedule_step" in g]
        if ts and self._lr_schedule is not None:
            self.set_schedule_step(int(ts[0]))

    def _adopt_momentum(self):
        """Loaded momentum buffers are fresh tensors, while a replayed hipGraph step reads and writes
        the arena's momentum storage: copy them into their arena views now (not at the next eager
        step), so a replay after ``load_state_dict`` continues from the loaded state."""
        a = self._arena
        if a is None or a.momentum is None:
            return
        views = a.momentum_views()
        with torch.no_grad():
            for p in a.params:
                st = self.state.get(p)
                b = st.get("momentum_buffer") if st else None
                if b is not None and b.data_ptr() != views[p._cdp_index].data_ptr():
                    views[p._cdp_index].copy_(b)
                    st["momentum_buffer"] = views[p._cdp_index]

    # ------------------------------------------------------------------ learning-rate schedule
    @property
    def lr_schedule(self):
        """The :class:`LRSchedule` as last set; None when the optimizer has none."""
        return self._lr_schedule

    @property
    def schedule_step(self):
        """The schedule's step index ``t`` (the ``step()`` calls so far): a 0-dim int64 device view the
        fused step advances itself (reading it here never syncs); None without ``lr_schedule``."""
        return self._sched_state[0] if self._sched_state is not None else None

    @property
    def last_lr(self):
        """The rate of the last step for param group 0 (0-dim float32 device view); None without
        ``lr_schedule``."""
        return self._sched_last[0] if self._sched_last is not None else None

    def _sched_check(self, what):
        if self._lr_schedule is None:
            raise RuntimeError(f"{what}: the optimizer was built without lr_schedule")
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{what} writes or reads the schedule's device words: not while the stream is capturing")

    def set_schedule_step(self, t: int):
        """Continue the schedule from step ``t`` (also zeroes the arrival word of the fused step's
        advance): in place, so a captured step follows at its next replay. Not while capturing."""
        self._sched_check("set_schedule_step")
        if int(t) != t or t < 0:
            raise ValueError(f"Invalid schedule step: {t}")
        self._sched_state[0:1].fill_(int(t))
        self._sched_state[1:2].fill_(0)

    def set_lr_schedule(self, sched: LRSchedule):
        """Replace the schedule of an optimizer built with one: the device configuration is refilled in
        place, so a captured step uses the new schedule at its next replay; ``t`` stays. Not while
        capturing."""
        self._sched_check("set_lr_schedule")
        if not isinstance(sched, LRSchedule):
            raise TypeError(f"lr_schedule must be an LRSchedule, not {type(sched).__name__}")
        self._lr_schedule = sched
        if self._sched_cfg is not None:
            self._sched_cfg.copy_(_native.lib().lr_sched_pack(*sched._pack_args()))

    def lr_schedule_table(self, first: int, n: int) -> torch.Tensor:
        """float32 ``[n]``: the rates of steps ``first .. first + n - 1`` for param group 0 at its current
        base rate (``lr_tensor`` when there is one), as the fused step evaluates them (on the device
        where the parameters are; from :meth:`LRSchedule.factor` otherwise)."""
        if self._lr_schedule is None:
            raise RuntimeError("lr_schedule_table: the optimizer was built without lr_schedule")
        if first < 0 or n < 0:
            raise ValueError(f"lr_schedule_table: first >= 0 and n >= 0 required, got {first}, {n}")
        base = self.param_groups[0]["lr"]
        if self._sched_cfg is not None and not _native.force_reference():
            return _native.lib().lr_sched_table(self._sched_cfg, self._lr_tensor, base, int(first), int(n))
        return torch.tensor([self._lr_schedule.rate(base, first + i) for i in range(n)], dtype=torch.float32,
                            device=self._sched_last.device)

    def _sched_kw(self, advance: bool) -> dict:
        """The schedule block of one fused launch; ``advance``: it is the last launch of this step()."""
        if self._sched_cfg is None:
            return {}
        # last_lr is group 0's rate: only its launches record theirs
        return dict(sched_state=self._sched_state, sched_cfg=self._sched_cfg,
                    sched_last=self._sched_last if self._sched_gi == 0 else None, sched_advance=bool(advance))

    def _sched_take_advance(self) -> bool:
        """True once per step(), for the launch that advances t: only in the last group with work."""
        if self._sched_pending and self._sched_take:
            self._sched_pending = False
            return True
        return False

    def _lr_of(self, group) -> float:
        """The rate of this step for ``group`` on the reference paths (CPU, ``force_reference``,
        per-parameter torch ops): ``group["lr"]``, or with a schedule ``float32(lr * factor(t))`` with t
        read on the host."""
        if self._lr_schedule is None:
            return group["lr"]
        if self._sched_host is None:
            if self._sched_state.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("lr_schedule: this step runs on a reference path, which reads the schedule's "
                                   "step on the host: not while the stream is capturing")
            t = int(self._sched_state[0])
            self._sched_host = (t, self._lr_schedule.factor(t))
        return torch.tensor(float(group["lr"]) * self._sched_host[1], dtype=torch.float64).to(torch.float32).item()

    def _sched_finish_step(self):
        """The advance of t when no fused launch took it (nothing launched, reference paths)."""
        if not self._sched_pending:
            return
        self._sched_pending = False
        st = self._sched_state
        if self._sched_host is None and self._sched_cfg is not None and not _native.force_reference():
            _native.lib().lr_sched_advance(st, self._sched_cfg, self._sched_last, self._lr_tensor,
                                           self.param_groups[0]["lr"])
            return
        self._sched_last.fill_(self._lr_of(self.param_groups[0]))
        st[0:1] += 1
        st[1:2].fill_(0)

    def state_dict(self):
        """torch's, and with a schedule ``param_groups[i]["lr_schedule_step"] = t`` (one host read: not
        while capturing). The extra key is inert in ``torch.optim.SGD.load_state_dict``."""
        sd = super().state_dict()
        if self._lr_schedule is not None:
            self._sched_check("state_dict")
            t = int(self._sched_state[0])
            for g in sd["param_groups"]:
                g["lr_schedule_step"] = t
        return sd

    # ------------------------------------------------------------------ weight EMA
    @property
    def ema_decay(self):
        """The EMA decay ``d`` as last set (the host value); None when the EMA is off."""
        return self._ema_decay

    def set_ema_decay(self, decay: float):
        """Change the decay of an optimizer built with ``ema_decay``: the two device coefficients are
        refilled in place, so a captured step uses the new value at its next replay (a decay warm-up
        without re-capture, as ``lr_tensor`` does for the learning rate). Not while capturing."""
        if self._ema_decay is None:
            raise RuntimeError("set_ema_decay: the optimizer was built without ema_decay")
        _check_ema_decay(decay)
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("set_ema_decay fills the device coefficients: not while the stream is capturing")
        d = float(decay)
        self._ema_decay = d
        self._ema_d = torch.tensor(d, dtype=torch.float32).item()
        self._ema_omd = torch.tensor(1.0 - d, dtype=torch.float32).item()  # the subtraction in double
        if self._ema_coef is not None:
            self._ema_coef[0:1].fill_(self._ema_d)
            self._ema_coef[1:2].fill_(self._ema_omd)

    @torch.no_grad()
    def reset_ema(self):
        """``e <- w`` for every parameter (e.g. after loading model weights)."""
        if self._ema_decay is None:
            raise RuntimeError("reset_ema: the optimizer was built without ema_decay")
        a = self._arena
        if a is not None:
            a.ema_buffer().copy_(a.data)
            views = a.ema_views()
        for g in self.param_groups:
            for p in g["params"]:
                if a is not None and getattr(p, "_cdp_arena", None) is a:
                    self.state[p]["ema_buffer"] = views[p._cdp_index]
                else:
                    self.state[p]["ema_buffer"] = p.detach().clone(memory_format=torch.preserve_format)

    @torch.no_grad()
    def _adopt_ema(self):
        """After ``load_state_dict``: loaded EMA buffers are copied into their arena views (which a
        replayed step reads and writes), as ``_adopt_momentum`` does; a parameter whose loaded state
        has none starts again from its current weight."""
        if self._ema_decay is None:
            return
        a = self._arena
        views = a.ema_views() if a is not None else None
        for g in self.param_groups:
            for p in g["params"]:
                st = self.state[p]
                b = st.get("ema_buffer")
                home = views[p._cdp_index] if a is not None and getattr(p, "_cdp_arena", None) is a else None
                if b is None:
                    if home is not None:
                        home.copy_(p.detach())
                        b = home
                    else:
                        b = p.detach().clone(memory_format=torch.preserve_format)
                elif home is not None and b.data_ptr() != home.data_ptr():
                    home.copy_(b)
                    b = home
                elif home is None:
                    b = b.detach().clone(memory_format=torch.preserve_format)  # never another optimizer's tensor
                st["ema_buffer"] = b

    def ema_state(self) -> dict:
        """``{parameter: its EMA}`` (the live tensors: arena views where the parameters are)."""
        if self._ema_decay is None:
            raise RuntimeError("ema_state: the optimizer was built without ema_decay")
        return {p: self.state[p]["ema_buffer"] for g in self.param_groups for p in g["params"]}

    @contextlib.contextmanager
    def ema_weights(self):
        """Evaluate with the averaged weights: the contents of the parameters and of their EMA are
        exchanged on entry and exchanged back on exit (bitwise, so training continues as if nothing
        happened). The weight products of the fused step are refreshed (or dropped) both times, since
        writes through the flat storage bump no parameter version. BatchNorm running statistics are
        not averaged: the EMA weights evaluate with the live buffers. Not while capturing."""
        if self._ema_decay is None:
            raise RuntimeError("ema_weights: the optimizer was built without ema_decay")
        self._ema_swap()
        try:
            yield self
        finally:
            self._ema_swap()

    @torch.no_grad()
    def _ema_swap(self):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ema_weights exchanges the weights with torch ops: not while the stream is capturing")
        a = self._arena
        if a is not None:
            e = a.ema_buffer()
            tmp = a.data.clone()
            a.data.copy_(e)
            e.copy_(tmp)
            if not a.prep_refresh():
                a.prep_valid = None
        for g in self.param_groups:
            for p in g["params"]:
                if a is not None and getattr(p, "_cdp_arena", None) is a:
                    continue
                e = self.state[p]["ema_buffer"]
                tmp = p.detach().clone(memory_format=torch.preserve_format)
                p.copy_(e)  # bumps the version: an eager forward prepares the weight anew
                e.copy_(tmp)

    def _ema_apply_reference(self, p):
        """The EMA of one parameter with torch ops, after its update (the arithmetic of the kernels)."""
        self.state[p]["ema_buffer"].mul_(self._ema_d).add_(p, alpha=self._ema_omd)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if getattr(self, "_ema_decay", None) is not None:  # not the constructor's own calls
            with torch.no_grad():
                for p in self.param_groups[-1]["params"]:
                    self.state[p]["ema_buffer"] = p.detach().clone(memory_format=torch.preserve_format)
            self._adopt_ema()  # into the arena where the parameter is in it

    # ------------------------------------------------------------------ fused weight preparation
    def refresh_weight_prep(self) -> bool:
        """Re-derive the next forward's weight |max| / W^T from the current weights (in place).

        With ``fused_prep`` (default) the step itself writes them for the next forward. Eager forwards
        notice weights edited since (a bumped version) and prepare them anew; a replayed hipGraph
        cannot, so after editing weights between replays of a captured step call this first."""
        return self._arena.prep_refresh() if self._arena is not None else False

    # ------------------------------------------------------------------ device-side LR
    def lr_tensor(self) -> torch.Tensor:
        """A 1-element device tensor holding the LR of param group 0 (graph-capture friendly)."""
        if self._lr_tensor is None:
            dev = self.param_groups[0]["params"][0].device
            self._lr_tensor = torch.tensor([self.param_groups[0]["lr"]], dtype=torch.float32, device=dev)
        return self._lr_tensor

    def sync_lr_tensor(self):
        if self._lr_tensor is not None:
            self._lr_tensor.fill_(self.param_groups[0]["lr"])

    # ------------------------------------------------------------------ zero_grad
    def zero_grad(self, set_to_none: bool = True):
        # set_to_none (torch's default) lets the next backward's kernels write each gradient straight
        # into its arena slot, which autograd then adopts as p.grad without a copy (FlatArena.claim).
        super().zero_grad(set_to_none=set_to_none)
        if self._arena is not None:
            self._arena.reset_claims()

    # ------------------------------------------------------------------ step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._overlap is not None:
            ov, self._overlap = self._overlap, None
            done = ov["reducer"].stepped_buckets()
            if done == ov["n"]:
                self._finish_overlapped(ov)
                self._run_post_step_joins()
                return loss
            if done:
                raise RuntimeError(f"overlapped optimizer step: only {done} of {ov['n']} buckets were stepped")
        self._counter_pending = self._step_counter
        self._sched_pending = self._lr_schedule is not None
        self._sched_host = None
        skip = False
        self._clip_fused = False
        if self._clip_enabled:
            # the norm is over the whole model: inside the one flat launch where the step is one (see
            # _flat_step), otherwise up front with torch ops
            self._clip_fused = self._clip_fusable()
            if not self._clip_fused:
                with_grad = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
                skip = bool(with_grad) and self._clip_reference(with_grad)
        self._begin_step()
        last_gi = -1
        if self._sched_pending and not skip:
            last_gi = max((gi for gi, g in enumerate(self.param_groups) if any(p.grad is not None for p in g["params"])),
                          default=-1)
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"] if p.grad is not None]
            if not params or skip:
                continue
            self._sched_take = gi == last_gi  # the step()'s last launch advances the schedule
            self._sched_gi = gi
            if self._arena is not None:
                self._arena.prep_valid = None  # re-marked below only by a fused step
            if params[0].is_cuda and not _native.force_reference():
                self._step_native(gi, group, params)
            else:
                self._step_reference(group, params)
        if self._counter_pending is not None:  # no fused launch took it (per-tensor / reference paths)
            c = self._counter_pending
            if c.is_cuda and not _native.force_reference():
                _native.lib().counter_inc(c)
            else:
                c += 1
            self._counter_pending = None
        self._end_step(skip)
        self._sched_finish_step()  # no fused launch took it (nothing launched / reference paths)
        self._steps += 1
        self._run_post_step_joins()
        return loss

    def _begin_step(self):
        """Per-step planning of a subclass, after the clip's and before the first group's launch."""

    def _end_step(self, skipped: bool):
        """Per-step bookkeeping of a subclass, after the last group's launch (``skipped``: the up-front clip
        of the reference paths left the step out)."""

    def _flat_step_extra(self, C, arena, s, e, plan) -> dict:
        """Further launches before, and keyword arguments of, the flat step's kernel (LARS)."""
        return {}

    _prep_cut = False  # whether the weight-preparation plan's rest chunks are cut at parameter boundaries

    def add_post_step_join(self, fn):
        """Run ``fn()`` at the end of every ``step()`` (e.g. to order the current stream after
        communication issued during backward; see ``DistributedDataParallel.early_buffer_broadcast``)."""
        if fn not in self._post_step_joins:
            self._post_step_joins.append(fn)

    def _run_post_step_joins(self):
        for fn in getattr(self, "_post_step_joins", ()):
            fn()

    # ------------------------------------------------------------------ overlapped step (DDP)
    def bucket_steps(self, ranges, reducer):
        """Split this iteration's step over gradient buckets (``DistributedDataParallel.overlap_optimizer``).

        ``ranges``: the buckets' flat arena ranges in launch order. Returns one keyword dict per
        bucket for the reducer's ``set_bucket_step`` -- the SGD of that range, run on the reducer's
        step stream right after the bucket's all-reduce -- or None when the step cannot be split
        this iteration (several param groups, parameters outside one arena run, first and later
        momentum steps mixed, no native kernels, ``max_grad_norm`` / ``skip_nonfinite``, ``ema_decay`` or
        ``lr_schedule`` set: the step then runs whole at ``step()``). The next ``step()`` then only does the
        bookkeeping, provided the reducer stepped every bucket; hyperparameters are those at the
        time of this call (the forward), the first-step momentum rule (buf = d_p) is kept."""
        if self._arena is None or len(self.param_groups) != 1 or _native.force_reference():
            return None
        if self._clip_enabled:
            return None  # the clip needs the norm of the whole model: the step runs whole at step()
        if self._ema_decay is not None:
            return None  # the per-bucket launches carry no EMA: the step runs whole at step()
        if self._lr_schedule is not None:
            return None  # the per-bucket launches carry no schedule: the step runs whole at step()
        group = self.param_groups[0]
        params, arena = group["params"], self._arena
        if len(params) != len(arena.params) or any(not p.is_cuda for p in params):
            return None
        rng = arena.contiguous_range(params)
        ranges = [(int(s), int(e)) for s, e in ranges]
        if rng is None or not ranges or ranges[0][0] != rng[0] or ranges[-1][1] != rng[1]:
            return None
        if any(ranges[k][1] != ranges[k + 1][0] for k in range(len(ranges) - 1)):
            return None
        m = group["momentum"]
        first = True
        if m != 0.0:
            mviews = arena.momentum_views()
            bufs = [self.state[p].get("momentum_buffer") for p in params]
            if any(b is not None and b.data_ptr() != mviews[p._cdp_index].data_ptr() for b, p in zip(bufs, params)):
                return None  # e.g. loaded buffers not yet adopted: a normal step moves them in
            firsts = [b is None for b in bufs]
            if any(firsts) and not all(firsts):
                return None
            first = all(firsts)
        plan = arena.prep_plan_ranges(ranges) if self.fused_prep else None
        mom = arena.momentum_buffer() if m != 0.0 else None
        lr_t = self._lr_tensor
        out = []
        for k, (s, e) in enumerate(ranges):
            a = dict(p=arena.data[s:e], g=arena.grad[s:e], buf=mom[s:e] if mom is not None else None, lr_t=lr_t,
                     lr=group["lr"], momentum=m, dampening=group["dampening"], wd=group["weight_decay"],
                     nesterov=group["nesterov"], first=first, maximize=group["maximize"],
                     counter=self._step_counter if k == len(ranges) - 1 else None)
            sub = plan["subs"][k] if plan is not None else None
            if sub is not None:
                a.update(desc=sub["desc"], meta=sub["meta"], amax=plan["amax"])
            out.append(a)
        self._overlap = {"reducer": reducer, "n": len(out), "first": first and m != 0.0, "prep": plan is not None,
                         "params": list(params)}
        return out

    def cancel_bucket_steps(self):
        self._overlap = None

    def _finish_overlapped(self, ov):
        """Bookkeeping of a step the reducer ran bucket by bucket (no kernel here)."""
        arena = self._arena
        if ov["first"]:
            mviews = arena.momentum_views()
            for p in ov["params"]:
                self.state[p]["momentum_buffer"] = mviews[p._cdp_index]
        arena.prep_valid = None
        if ov["prep"]:
            arena.prep_mark_valid()
        self._counter_pending = None  # advanced by the last bucket's kernel
        self._steps += 1

    def advance_each_step(self, counter: torch.Tensor):
        """Advance ``counter`` (a device int64 step counter, e.g. a DeviceLoader's) by one in every
        ``step()``, inside the SGD kernel itself: one dispatch less per training step. Only for
        loops that fetch exactly one batch per optimizer step; ``None`` stops it."""
        self._step_counter = counter

    def _first_flags(self, params):
        firsts = [self.state[p].get("momentum_buffer") is None for p in params]
        return firsts

    def _step_native(self, gi, group, params):
        C = _native.lib()
        lr, m, damp, wd = group["lr"], group["momentum"], group["dampening"], group["weight_decay"]
        nest, maxim = group["nesterov"], group["maximize"]
        lr_t = self._lr_tensor if (gi == 0 and self._lr_tensor is not None) else None
        arena = self._arena
        rng = None
        if arena is not None and len(params) == len(group["params"]):
            rng = arena.contiguous_range(params)
            if rng is not None:
                arena.ensure_grads_in_arena(params)
        if rng is not None and m != 0.0:
            # momentum buffers must be the arena's views (first step: buf = d_p)
            firsts = self._first_flags(params)
            mom = arena.momentum_buffer()
            mviews = arena.momentum_views()
            consistent = all(
                (self.state[p].get("momentum_buffer") is None)
                or self.state[p]["momentum_buffer"].data_ptr() == mviews[p._cdp_index].data_ptr()
                for p in params
            )
            if not consistent:
                # e.g. after load_state_dict: move loaded buffers into the arena
                for p in params:
                    b = self.state[p].get("momentum_buffer")
                    if b is not None:
                        mviews[p._cdp_index].copy_(b)
                        self.state[p]["momentum_buffer"] = mviews[p._cdp_index]
                firsts = self._first_flags(params)
            if all(firsts) or not any(firsts):
                s, e = rng
                self._flat_step(C, arena, s, e, mom[s:e], lr_t, lr, m, damp, wd, nest, all(firsts), maxim)
                if all(firsts):
                    for p in params:
                        self.state[p]["momentum_buffer"] = mviews[p._cdp_index]
                return
        elif rng is not None and m == 0.0:
            s, e = rng
            self._flat_step(C, arena, s, e, None, lr_t, lr, 0.0, damp, wd, nest, True, maxim)
            return
        # general path: one launch per parameter (non-arena / partial groups)
        if self._clip_fused:
            raise RuntimeError("gradient clipping was planned into a flat step that did not run")
        for k, p in enumerate(params):
            st = self.state[p]
            buf = st.get("momentum_buffer")
            first = buf is None
            # the schedule: every launch reads t, the last one of the step() advances it
            sched = self._sched_kw(k == len(params) - 1 and self._sched_take_advance())
            if m != 0.0 and first:
                buf = torch.empty_like(p, memory_format=torch.contiguous_format)
            pv = p.data if p.data.is_contiguous() else None
            g = p.grad
            ema = {}
            eb = st["ema_buffer"] if self._ema_decay is not None else None  # each parameter's own EMA
            if eb is not None:
                ec = eb.contiguous()
                ema = dict(ema=ec.view(-1), ema_coef=self._ema_coef)
            if pv is None or not g.is_contiguous():
                # strided (channels_last) tensors: update through flat contiguous copies
                pc = p.data.contiguous()
                gc = g.contiguous()
                bc = buf.contiguous() if buf is not None else None
                C.sgd_step(pc.view(-1), gc.view(-1), bc.view(-1) if bc is not None else None, lr_t, lr, m, damp, wd,
                           1.0, nest, first, maxim, **ema, **sched)
                p.data.copy_(pc)
                if buf is not None and bc is not buf:
                    buf.copy_(bc)
            else:
                C.sgd_step(pv.view(-1), g.view(-1), buf.view(-1) if buf is not None else None, lr_t, lr, m, damp,
                           wd, 1.0, nest, first, maxim, **ema, **sched)
            if eb is not None and ec is not eb:
                eb.copy_(ec)
            if m != 0.0:
                st["momentum_buffer"] = buf

    def _flat_step(self, C, arena, s, e, mom, lr_t, lr, m, damp, wd, nest, first, maxim):
        """One launch over the arena range: plain SGD, or SGD that also writes the next forward's
        weight |max| partials and W^T (FlatArena.prep_plan_for) when a model registered them."""
        plan = arena.prep_plan_for(s, e, cut=self._prep_cut) if self.fused_prep else None
        ctr, self._counter_pending = self._counter_pending, None
        clip = {}
        if self._clip_fused:
            # one extra dispatch: the partial sums of squares of the whole range (the arena's pad
            # floats are zero); every SGD launch below derives the same norm / coefficient from them
            # in its prologue. p.grad itself is left unscaled.
            part = self._clip_part[:C.grad_norm_parts(e - s)]
            C.grad_sumsq(arena.grad[s:e], part)
            clip = dict(clip_part=part, max_norm=self.max_grad_norm if self.max_grad_norm is not None else float("inf"),
                        stats=self._clip_stats, skip_nonfinite=self.skip_nonfinite)
        clip.update(self._flat_step_extra(C, arena, s, e, plan))
        ema = arena.ema_buffer() if self._ema_decay is not None else None  # state[p]["ema_buffer"] are its views
        if ema is not None:
            clip.update(ema=ema[s:e], ema_coef=self._ema_coef)
        adv = self._sched_take_advance()
        if plan is not None and "subs" in plan:
            clip.update(self._sched_kw(False))  # several launches: only the last advances t (below)
        else:
            clip.update(self._sched_kw(adv))
        if plan is None:
            C.sgd_step(arena.data[s:e], arena.grad[s:e], mom, lr_t, lr, m, damp, wd, 1.0, nest, first, maxim, ctr,
                       **clip)
            return
        if "subs" in plan:  # the split plan of an overlapped step (same buffers): its ranges in turn
            last = len(plan["ranges"]) - 1
            for k, ((a, b), sub) in enumerate(zip(plan["ranges"], plan["subs"])):
                mk = mom[a - s:b - s] if mom is not None else None
                c = ctr if k == last else None
                ck = clip if k == last or not clip else dict(clip, stats=None)  # stats written once
                if ema is not None:
                    ck = dict(ck, ema=ema[a:b])
                if adv and k == last:
                    ck = dict(ck, sched_advance=True)
                if sub is None:
                    C.sgd_step(arena.data[a:b], arena.grad[a:b], mk, lr_t, lr, m, damp, wd, 1.0, nest, first, maxim, c,
                               **ck)
                else:
                    C.sgd_step_prep(arena.data[a:b], arena.grad[a:b], mk, lr_t, lr, m, damp, wd, 1.0, nest, first,
                                    maxim, sub["desc"], sub["meta"], plan["amax"], c, **ck)
            arena.prep_mark_valid()
            return
        C.sgd_step_prep(arena.data[s:e], arena.grad[s:e], mom, lr_t, lr, m, damp, wd, 1.0, nest, first, maxim,
                        plan["desc"], plan["meta"], plan["amax"], ctr, **clip)
        arena.prep_mark_valid()

    def _step_reference(self, group, params):
        wd = group["weight_decay"]
        for p in params:
            d_p = p.grad if not group["maximize"] else -p.grad
            if wd != 0:
                d_p = d_p.add(p, alpha=wd)
            self._apply_reference(group, p, d_p)

    def _apply_reference(self, group, p, d_p):
        """Momentum, dampening, Nesterov and ``p -= lr * d_p`` for one parameter, with torch ops."""
        lr, m, damp = self._lr_of(group), group["momentum"], group["dampening"]
        if m != 0:
            st = self.state[p]
            buf = st.get("momentum_buffer")
            if buf is None:
                buf = torch.clone(d_p).detach()
                st["momentum_buffer"] = buf
            else:
                buf.mul_(m).add_(d_p, alpha=1 - damp)
            d_p = d_p.add(buf, alpha=m) if group["nesterov"] else buf
        p.add_(d_p, alpha=-lr)
        if self._ema_decay is not None:
            self._ema_apply_reference(p)


class LARS(SGD):
    """:class:`SGD` with layer-wise adaptive rate scaling (You, Gitman, Ginsburg, "Large Batch Training
    of Convolutional Networks"): every adapted parameter tensor ``w`` with scaled gradient
    ``g^ = grad_scale * clip_coef * g`` is stepped with ``q * (g^ + wd * w)`` in place of
    ``g^ + wd * w``, where

        ``q = trust_coefficient * |w| / (|g^| + wd * |w| + eps)``  (1 when ``|w|`` or ``|g^|`` is 0)

    is evaluated in fp64 from fp64 sums of squares and rounded once to fp32. A parameter is adapted
    and decayed when ``w.ndim > 1`` or ``exclude_bias_and_norm`` is false; with the default exclusion
    biases and BatchNorm weights get ``q = 1`` and no weight decay (the usual recipe), so the whole
    model stays one param group and one flat launch. Momentum, dampening, Nesterov, ``maximize``,
    ``max_grad_norm`` / ``skip_nonfinite``, ``ema_decay``, ``lr_schedule`` (warm-up and polynomial decay
    evaluated inside the step) and the device-side base rate (``lr_tensor``) are :class:`SGD`'s.
    ``trust_coefficient``, ``eps`` and ``exclude_bias_and_norm`` are ``param_groups`` entries. The defaults 0.001 and 1e-8 are the conventional ones of the paper
    and common implementations; nothing was measured to choose them.

    MI355X path, where the step is one flat launch over an arena range (the conditions of the fused
    clip): one extra dispatch writes per-parameter fp64 partial sums of squares of weights and
    gradients (``csrc/kernels/lars.hip``), and every workgroup of the SGD kernel, which then owns
    elements of exactly one parameter, derives that parameter's ``q`` from them in its prologue: no
    host sync, no atomics, so a captured hipGraph step adapts with each replay's own norms. Every
    other case (CPU, ``force_reference``, several groups, parameters outside the arena) evaluates the
    same formula per parameter with torch ops. ``bucket_steps`` declines, so under
    ``DistributedDataParallel.overlap_optimizer`` the step runs whole at ``step()``.
    """

    def __init__(
        self,
        params,
        lr: float,
        momentum: float = 0.0,
        dampening: float = 0.0,
        weight_decay: float = 0.0,
        nesterov: bool = False,
        *,
        trust_coefficient: float = 0.001,
        eps: float = 1e-8,
        exclude_bias_and_norm: bool = True,
        maximize: bool = False,
        flat: bool = True,
        max_grad_norm: float | None = None,
        skip_nonfinite: bool = False,
        ema_decay: float | None = None,
        lr_schedule: LRSchedule | None = None,
    ):
        if not float(trust_coefficient) >= 0.0:
            raise ValueError(f"Invalid trust_coefficient: {trust_coefficient}")
        if not float(eps) >= 0.0:
            raise ValueError(f"Invalid eps: {eps}")
        self._extra_defaults = dict(trust_coefficient=float(trust_coefficient), eps=float(eps),
                                    exclude_bias_and_norm=bool(exclude_bias_and_norm))
        super().__init__(params, lr, momentum, dampening, weight_decay, nesterov, maximize=maximize, flat=flat,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, ema_decay=ema_decay,
                         lr_schedule=lr_schedule)
        all_params = [p for g in self.param_groups for p in g["params"]]
        self._slot = {id(p): k for k, p in enumerate(all_params)}
        # allocated here, never inside a capture
        self._trust = torch.ones(len(all_params), dtype=torch.float32, device=all_params[0].device)
        self._lars_fused = False
        self._lars_plan = None  # (key, plan) of the norms pass, per arena layout and form of the step

    _prep_cut = True

    @property
    def trust_ratios(self) -> torch.Tensor:
        """``q`` of every parameter at the last step, in ``param_groups`` order (1.0 for excluded
        parameters): a device tensor the step writes; reading it here never syncs."""
        return self._trust

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_trust"):  # not the constructor's own calls
            all_params = [p for g in self.param_groups for p in g["params"]]
            self._slot = {id(p): k for k, p in enumerate(all_params)}
            t = torch.ones(len(all_params), dtype=torch.float32, device=self._trust.device)
            t[:self._trust.numel()] = self._trust
            self._trust = t

    def _on_relayout(self, arena):
        super()._on_relayout(arena)
        self._lars_plan = None  # offsets moved: the work list is stale

    def bucket_steps(self, ranges, reducer):
        """None: the per-bucket split of an overlapped step is not offered (the norms are local to a
        parameter, so it is possible; until then the step runs whole at ``step()``), with or without an
        ``lr_schedule``."""
        return None

    def _begin_step(self):
        self._lars_fused = self._flat_fusable()
        if self._lars_fused and self._clip_enabled and not self._clip_fused:
            self._lars_fused = False  # the clip already scaled the gradients with torch ops

    def _step_native(self, gi, group, params):
        if not self._lars_fused:
            return self._step_reference(group, params)  # the per-parameter launches know no trust ratio
        done = self._steps_flat
        super()._step_native(gi, group, params)
        if self._steps_flat == done:
            raise RuntimeError("LARS was planned into a flat step that did not run")

    _steps_flat = 0

    def _flat_step_extra(self, C, arena, s, e, plan):
        self._steps_flat += 1
        if not self._lars_fused:
            return {}
        if plan is not None and "subs" in plan:
            raise RuntimeError("LARS cannot run over the split plan of an overlapped step")
        group = self.param_groups[0]
        lp = self._lars_plan_for(C, arena, s, e, plan)
        # one extra dispatch: {sum w^2, sum g^2} of every (parameter, chunk); the workgroups of the
        # step below add their own parameter's pairs in their prologue
        C.lars_norms(arena.data[s:e], arena.grad[s:e], lp["desc"], lp["meta"], lp["part"])
        return dict(lars=C.LarsStep(desc=lp["desc"], meta=lp["meta"], part=lp["part"], ratios=self._trust,
                                    trust_coefficient=group["trust_coefficient"], eps=group["eps"],
                                    exclude=group["exclude_bias_and_norm"]))

    def _lars_plan_for(self, C, arena, s, e, plan):
        """The norms work list over [s, e), with the owners of the weight-preparation plan's
        workgroups when the step runs in that form. Built once per arena layout (and form), outside
        any capture, like the weight-preparation plan itself."""
        key = (arena.layout_gen, s, e, id(plan["desc"]) if plan is not None else None)
        if self._lars_plan is not None and self._lars_plan[0] == key:
            return self._lars_plan[1]
        idx = [i for i, off in enumerate(arena.offsets) if s <= off < e]
        ps = [arena.params[i] for i in idx]
        r = C.lars_plan(arena.data, s, e, [arena.offsets[i] for i in idx], [arena.numels[i] for i in idx],
                        [p.dim() for p in ps], [self._slot[id(p)] for p in ps],
                        plan["desc"] if plan is not None else None, plan["meta"] if plan is not None else None)
        lp = {"desc": r[0], "meta": r[1], "part": r[2], "prep_desc": plan["desc"] if plan is not None else None}
        self._lars_plan = (key, lp)
        return lp

    def _step_reference(self, group, params):
        wd, eta, eps = group["weight_decay"], group["trust_coefficient"], group["eps"]
        for p in params:
            g = p.grad
            k = self._slot[id(p)]
            if p.dim() > 1 or not group["exclude_bias_and_norm"]:
                wn = p.detach().double().square().sum().sqrt()
                gn = g.double().square().sum().sqrt()
                q = eta * wn / (gn + wd * wn + eps)
                q = torch.where((wn == 0) | (gn == 0), torch.ones_like(q), q).float()
                self._trust[k].copy_(q)
                d_p = g * q  # gs_eff = q: the reference paths scale p.grad itself by grad_scale * coef
                if group["maximize"]:
                    d_p = -d_p
                if wd != 0:
                    d_p = torch.addcmul(d_p, p, q * wd)
            else:
                self._trust[k].fill_(1.0)
                d_p = g if not group["maximize"] else -g
            self._apply_reference(group, p, d_p)


class AdamW(SGD):
    """AdamW (decoupled weight decay, ``torch.optim.AdamW``'s semantics) over the flat arenas, with everything
    the SGD family offers (``max_grad_norm`` / ``skip_nonfinite``, ``ema_decay``, ``lr_schedule``, ``lr_tensor``,
    ``advance_each_step``, ``add_post_step_join``, the reducer's relayout) under the same names. For the step
    count ``t`` (the steps taken so far) and ``T = t + 1``:

        ``m = b1 m + (1 - b1) g``, ``v = b2 v + (1 - b2) g^2``,
        ``a = (m / (1 - b1^T)) / (sqrt(v) / sqrt(1 - b2^T) + eps)``, ``w -= lr (a + wd w)``

    (``w - lr (a + wd w)`` is torch's ``w (1 - lr wd) - lr a``). ``param_groups`` carry exactly the keys of the
    installed ``torch.optim.AdamW`` and the per-parameter state is ``step``, ``exp_avg``, ``exp_avg_sq``, so
    ``state_dict()`` loads into ``torch.optim.AdamW`` and the reverse (``ema_buffer`` and ``lr_schedule_step`` are
    inert there). ``amsgrad`` is not built.

    The step count lives on the device (``adam_step``, an int64 word allocated here): every workgroup of the
    fused kernel (``csrc/kernels/adam.hip``) reads it in its prologue, evaluates the bias corrections in fp64
    and the last launch of the step advances it by an arrival count, so a captured hipGraph step needs no host
    value; ``set_adam_step`` refills it in place. All parameters share the one ``t`` -- unlike torch, where a
    parameter without a gradient keeps its own count; ``state_dict()`` writes ``t`` into every ``step`` and
    ``load_state_dict()`` raises ``ValueError`` when the loaded ones disagree. A step skipped by
    ``skip_nonfinite`` leaves ``t``, ``m``, ``v``, ``w`` and the EMA bitwise unchanged (the learning-rate
    schedule's own counter still counts the iteration).

    ``exp_avg`` lives in the arena's momentum storage, ``exp_avg_sq`` in a second one beside it; one flat launch
    moves 28 bytes per element (36 with the EMA). The step does not emit the next forward's weight maxima and
    W^T as the fused SGD step does: the forward prepares its weights with its stand-alone launch (one more launch
    and one more read of the conv weights per step). ``bucket_steps`` declines, so under
    ``DistributedDataParallel.overlap_optimizer`` the step runs whole at ``step()``. CPU, ``force_reference``,
    several param groups' odd layouts and parameters outside one arena run evaluate the same formulas per
    parameter (torch ops, or one launch per parameter on the GPU). With ``eps = 0`` an element whose ``m`` and
    ``v`` are both zero gets ``a = 0`` from the kernels (the arena's pad floats stay zero) and ``0 / 0`` from the
    torch-op paths, as from torch."""

    _lamb = False

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, *,
                 amsgrad: bool = False, maximize: bool = False, flat: bool = True, max_grad_norm: float | None = None,
                 skip_nonfinite: bool = False, ema_decay: float | None = None, lr_schedule: LRSchedule | None = None):
        if amsgrad:
            raise ValueError("amsgrad=True is not built")
        if isinstance(lr, torch.Tensor):
            raise ValueError("a tensor lr is not supported: lr_tensor() is the device-side rate")
        # torch's own checks of lr, betas, eps and weight_decay (ValueError), and its param_group keys
        probe = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=betas, eps=eps,
                                  weight_decay=weight_decay, maximize=bool(maximize))
        self._check_common(max_grad_norm, ema_decay, lr_schedule)
        defaults = dict(probe.defaults)
        defaults.update(getattr(self, "_extra_defaults", {}))  # a subclass's own param_group entries (LAMB)
        Optimizer.__init__(self, params, defaults)
        self._init_common(flat, max_grad_norm, skip_nonfinite, ema_decay, lr_schedule)
        all_params = [p for g in self.param_groups for p in g["params"]]
        # {t, arrivals}: allocated here, never inside a capture
        self._adam_state = torch.zeros(2, dtype=torch.int64, device=all_params[0].device)
        self._adam_host = None  # t of this step() where a reference path read it
        self._adam_ref = self._adam_advanced = False
        self._adam_last_gi = -1
        self._lamb_fused = False

    # ------------------------------------------------------------------ the step count
    @property
    def adam_step(self):
        """The step count ``t`` (steps taken so far): a 0-dim int64 device view the fused step advances
        itself; reading it here never syncs."""
        return self._adam_state[0]

    def set_adam_step(self, t: int):
        """Continue from step count ``t`` (also zeroes the arrival word): in place, so a captured step follows
        at its next replay. Not while capturing."""
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("set_adam_step fills the device step count: not while the stream is capturing")
        if int(t) != t or t < 0:
            raise ValueError(f"Invalid step count: {t}")
        self._adam_state[0:1].fill_(int(t))
        self._adam_state[1:2].fill_(0)

    def _adam_t_host(self) -> int:
        if self._adam_host is None:
            if self._adam_state.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("this step runs on a reference path, which reads the step count on the host: "
                                   "not while the stream is capturing")
            self._adam_host = int(self._adam_state[0])
        return self._adam_host

    # ------------------------------------------------------------------ state
    def _state_of(self, p):
        """``state[p]`` with its moments: arena views where the parameter is in the arena (a tensor loaded
        from elsewhere is copied in), fresh zeros otherwise."""
        st = self.state[p]
        a = self._arena
        if a is not None and getattr(p, "_cdp_arena", None) is a:
            off = a.offsets[p._cdp_index]
            for key, buf in (("exp_avg", a.momentum_buffer()), ("exp_avg_sq", a.second_buffer())):
                b = st.get(key)
                if b is None or b.data_ptr() != buf.data_ptr() + off * buf.element_size():
                    home = _view_like(buf, off, p.data)
                    if b is not None:
                        home.copy_(b)
                    st[key] = home
        else:
            for key in ("exp_avg", "exp_avg_sq"):
                if st.get(key) is None:
                    st[key] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if "step" not in st:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)  # state_dict() writes t here
        return st

    def _on_relayout(self, arena):
        super()._on_relayout(arena)
        self._lamb_plan = None  # offsets moved: LAMB's work list is stale
        if arena is not self._arena:
            return
        mv = arena.momentum_views() if arena.momentum is not None else None
        sv = arena.second_views() if arena.second is not None else None
        for p in arena.params:
            st = self.state.get(p)
            if not st:
                continue
            if mv is not None and st.get("exp_avg") is not None:
                st["exp_avg"] = mv[p._cdp_index]
            if sv is not None and st.get("exp_avg_sq") is not None:
                st["exp_avg_sq"] = sv[p._cdp_index]

    def state_dict(self):
        """torch's: ``step`` of every parameter is ``t`` as the float32 0-dim tensor ``torch.optim.AdamW`` uses
        (one host read: not while capturing)."""
        if self._adam_state.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("state_dict reads the device step count: not while the stream is capturing")
        t = int(self._adam_state[0])
        for g in self.param_groups:
            for p in g["params"]:
                st = self.state.get(p)
                if st and "exp_avg" in st:
                    st["step"] = torch.tensor(float(t), dtype=torch.float32)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        steps = {int(float(st["step"])) for st in state_dict["state"].values() if "step" in st}
        if len(steps) > 1:
            raise ValueError(f"load_state_dict: the parameters' step counts disagree ({sorted(steps)}); "
                             "all parameters share one step count here")
        super().load_state_dict(state_dict)
        if steps:
            self.set_adam_step(steps.pop())
        # loaded moments are fresh tensors, while a replayed hipGraph step reads the arena's storages: move
        # them in now (as _adopt_momentum does for SGD); a parameter without loaded moments starts from zero
        a = self._arena
        with torch.no_grad():
            for g in self.param_groups:
                for p in g["params"]:
                    st = self.state.get(p)
                    if st and "exp_avg" in st:
                        self._state_of(p)
                    elif a is not None and getattr(p, "_cdp_arena", None) is a:
                        if a.momentum is not None:
                            a.momentum_views()[p._cdp_index].zero_()
                        if a.second is not None:
                            a.second_views()[p._cdp_index].zero_()

    def bucket_steps(self, ranges, reducer):
        """None: the per-bucket split of an overlapped step is not offered; the step runs whole at ``step()``."""
        return None

    # ------------------------------------------------------------------ step
    def _begin_step(self):
        self._adam_host = None
        self._adam_ref = self._adam_advanced = False
        self._adam_last_gi = max((gi for gi, g in enumerate(self.param_groups)
                                  if any(p.grad is not None for p in g["params"])), default=-1)
        if self._lamb:
            self._lamb_fused = self._flat_fusable()
            if self._lamb_fused and self._clip_enabled and not self._clip_fused:
                self._lamb_fused = False  # the clip already scaled the gradients with torch ops

    def _end_step(self, skipped):
        # the advance of t when no fused launch took it (reference paths); a skipped step did not happen
        if self._adam_ref and not self._adam_advanced and not skipped:
            self._adam_state[0:1] += 1

    def _step_native(self, gi, group, params):
        if self._lamb and not self._lamb_fused:
            return self._step_reference(group, params)  # the per-parameter launches know no trust ratio
        C = _native.lib()
        (b1, b2), eps, wd, maxim, lr = group["betas"], group["eps"], group["weight_decay"], group["maximize"], group["lr"]
        lr_t = self._lr_tensor if (gi == 0 and self._lr_tensor is not None) else None
        arena = self._arena
        last = gi == self._adam_last_gi  # the step()'s last launch advances t
        rng = None
        if arena is not None and len(params) == len(group["params"]):
            rng = arena.contiguous_range(params)
        if rng is not None:
            arena.ensure_grads_in_arena(params)
            for p in params:
                self._state_of(p)
            s, e = rng
            w, g = arena.data[s:e], arena.grad[s:e]
            m, v = arena.momentum_buffer()[s:e], arena.second_buffer()[s:e]
            ctr, self._counter_pending = self._counter_pending, None
            kw = {}
            if self._clip_fused:
                # one extra dispatch, as in the SGD step: the partial sums of squares of the whole range
                part = self._clip_part[:C.grad_norm_parts(e - s)]
                C.grad_sumsq(g, part)
                kw = dict(clip_part=part, max_norm=self.max_grad_norm if self.max_grad_norm is not None else float("inf"),
                          skip_nonfinite=self.skip_nonfinite)
            if self._lamb:
                lp = self._lamb_plan_for(C, arena, s, e)
                lamb = C.LambStep(desc=lp["desc"], meta=lp["meta"], part=lp["part"], ratios=self._trust,
                                  exclude=group["exclude_bias_and_norm"])
                # pass 1: the new m, v and {sum w^2, sum r^2} of every (parameter, chunk)
                C.lamb_moments(w, g, m, v, b1, b2, eps, wd, maxim, self._adam_state, lamb, **kw)
                kw["lamb"] = lamb
            if self._clip_fused:
                kw["stats"] = self._clip_stats
            if self._ema_decay is not None:
                kw.update(ema=arena.ema_buffer()[s:e], ema_coef=self._ema_coef)
            kw.update(self._sched_kw(self._sched_take_advance()))
            C.adam_step(w, g, m, v, lr_t, lr, b1, b2, eps, wd, maxim, self._adam_state, last, ctr, **kw)
            self._adam_advanced = self._adam_advanced or last
            return
        if self._clip_fused or self._lamb:
            raise RuntimeError("the step was planned into a flat launch that did not run")
        # general path: one launch per parameter (non-arena / partial groups)
        for k, p in enumerate(params):
            st = self._state_of(p)
            fin = k == len(params) - 1
            sched = self._sched_kw(fin and self._sched_take_advance())
            eb = st["ema_buffer"] if self._ema_decay is not None else None
            if arena is not None and getattr(p, "_cdp_arena", None) is arena:
                # the parameter's floats in the flat storages (its views share one layout)
                arena.ensure_grads_in_arena([p])
                o, n = arena.offsets[p._cdp_index], arena.numels[p._cdp_index]
                ema = dict(ema=arena.ema_buffer()[o:o + n], ema_coef=self._ema_coef) if eb is not None else {}
                C.adam_step(arena.data[o:o + n], arena.grad[o:o + n], arena.momentum_buffer()[o:o + n],
                            arena.second_buffer()[o:o + n], lr_t, lr, b1, b2, eps, wd, maxim, self._adam_state,
                            last and fin, **ema, **sched)
                continue
            # any other tensor: through flat contiguous copies where it is strided
            ts = [p.data, p.grad, st["exp_avg"], st["exp_avg_sq"]] + ([eb] if eb is not None else [])
            cs = [t.contiguous() for t in ts]
            ema = dict(ema=cs[4].view(-1), ema_coef=self._ema_coef) if eb is not None else {}
            C.adam_step(cs[0].view(-1), cs[1].view(-1), cs[2].view(-1), cs[3].view(-1), lr_t, lr, b1, b2, eps, wd, maxim,
                        self._adam_state, last and fin, **ema, **sched)
            for t, c in zip(ts, cs):
                if c is not t and t is not p.grad:
                    t.copy_(c)
        self._adam_advanced = self._adam_advanced or last

    _lamb_plan = None  # (key, plan) of LAMB's two passes, per arena layout

    def _lamb_plan_for(self, C, arena, s, e):
        """The (parameter, chunk) work list of LAMB's two passes over [s, e): ``lars_plan``'s, built once per
        arena layout, outside any capture."""
        key = (arena.layout_gen, s, e)
        if self._lamb_plan is not None and self._lamb_plan[0] == key:
            return self._lamb_plan[1]
        idx = [i for i, off in enumerate(arena.offsets) if s <= off < e]
        ps = [arena.params[i] for i in idx]
        r = C.lars_plan(arena.data, s, e, [arena.offsets[i] for i in idx], [arena.numels[i] for i in idx],
                        [p.dim() for p in ps], [self._slot[id(p)] for p in ps], None, None)
        lp = {"desc": r[0], "meta": r[1], "part": r[2]}
        self._lamb_plan = (key, lp)
        return lp

    def _step_reference(self, group, params):
        (b1, b2), eps, wd, maxim = group["betas"], group["eps"], group["weight_decay"], group["maximize"]
        lr = self._lr_of(group)
        T = self._adam_t_host() + 1
        bc1, bc2s = 1.0 - b1 ** T, math.sqrt(1.0 - b2 ** T)
        for p in params:
            st = self._state_of(p)
            m, v = st["exp_avg"], st["exp_avg_sq"]
            g = -p.grad if maxim else p.grad
            m.mul_(b1).add_(g, alpha=1.0 - b1)
            v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
            r = (m / bc1) / (v.sqrt() / bc2s).add_(eps)
            adapted = self._lamb and (p.dim() > 1 or not group["exclude_bias_and_norm"])
            if wd != 0 and (adapted or not self._lamb):
                r = r.add(p, alpha=wd)
            if self._lamb:
                k = self._slot[id(p)]
                if adapted:
                    wn = p.detach().double().square().sum().sqrt()
                    rn = r.double().square().sum().sqrt()
                    q = torch.where((wn == 0) | (rn == 0), torch.ones_like(wn), wn / rn).to(p.dtype)
                    self._trust[k].copy_(q)
                    r = r * q
                else:
                    self._trust[k].fill_(1.0)
            p.add_(r, alpha=-lr)
            if self._ema_decay is not None:
                self._ema_apply_reference(p)
        self._adam_ref = True


class LAMB(AdamW):
    """LAMB (You et al., "Large Batch Optimization for Deep Learning"): :class:`AdamW`'s moments with a
    layer-wise trust ratio over the Adam update. Per adapted parameter tensor

        ``r = m^ / (sqrt(v^) + eps) + wd w``, ``q = |w| / |r|`` (1 when ``|w|`` or ``|r|`` is 0), ``w -= lr q r``

    with the norms from fp64 sums of squares and ``q`` evaluated in fp64 and rounded once. There is NO clamp on
    ``q`` (neither the paper's optional ``phi`` nor the ``[0, 10]`` clip of some implementations). A parameter
    is adapted and decayed when ``w.ndim > 1`` or ``exclude_bias_and_norm`` (a ``param_groups`` entry) is
    false; with the default exclusion biases and BatchNorm weights get ``q = 1`` and no weight decay --
    :class:`LARS`'s rule, so the model stays one param group and one flat step. ``trust_ratios`` holds every
    parameter's ``q``. The defaults (``lr`` 1e-3, ``betas`` (0.9, 0.999), ``eps`` 1e-6, ``weight_decay`` 0.01) are
    the conventional ones of common implementations; nothing was measured to choose them.

    MI355X path, where the step is one flat range of the arena (the conditions of the fused clip): two launches
    over LARS's (parameter, chunk) work list. Pass 1 stores the new ``m``, ``v`` and each chunk's fp64 pair
    ``{sum w^2, sum r^2}``; pass 2 recomputes ``r`` from the new ``m``, ``v`` with the same function (the same
    bits: there is no arena for the update), derives its parameter's ``q`` from the pairs in its prologue and
    applies the update and the EMA: 40 bytes per element (48 with the EMA), no host sync, no atomics on data,
    so a captured hipGraph step adapts with each replay's own norms. Every other case evaluates the same
    formulas per parameter with torch ops. Everything else is :class:`AdamW`'s."""

    _lamb = True

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 0.01, *,
                 exclude_bias_and_norm: bool = True, amsgrad: bool = False, maximize: bool = False, flat: bool = True,
                 max_grad_norm: float | None = None, skip_nonfinite: bool = False, ema_decay: float | None = None,
                 lr_schedule: LRSchedule | None = None):
        self._extra_defaults = dict(exclude_bias_and_norm=bool(exclude_bias_and_norm))
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad=amsgrad, maximize=maximize, flat=flat,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, ema_decay=ema_decay,
                         lr_schedule=lr_schedule)
        all_params = [p for g in self.param_groups for p in g["params"]]
        self._slot = {id(p): k for k, p in enumerate(all_params)}
        # allocated here, never inside a capture
        self._trust = torch.ones(len(all_params), dtype=torch.float32, device=all_params[0].device)

    @property
    def trust_ratios(self) -> torch.Tensor:
        """``q`` of every parameter at the last step, in ``param_groups`` order (1.0 for excluded
        parameters): a device tensor the step writes; reading it here never syncs."""
        return self._trust

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_trust"):  # not the constructor's own calls
            all_params = [p for g in self.param_groups for p in g["params"]]
            self._slot = {id(p): k for k, p in enumerate(all_params)}
            t = torch.ones(len(all_params), dtype=torch.float32, device=self._trust.device)
            t[:self._trust.numel()] = self._trust
            self._trust = t


def _check_ema_decay(decay):
    d = float(decay)
    if math.isnan(d) or not 0.0 <= d <= 1.0:
        raise ValueError(f"Invalid ema_decay: {decay}")


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` (same signature, same return: the total norm as a tensor;
    gradients scaled in place) in two launches where it can be: for the 2-norm of GPU parameters whose
    gradients are one contiguous run of a :class:`~.utils.arena.FlatArena`, one kernel writes fp64
    partial sums of squares of the run and a second derives ``coef = min(max_norm / (norm + 1e-6), 1)``
    from them and scales the run. Anything else (another norm type, parameters outside an arena,
    CPU) is handed to torch's implementation. ``error_if_nonfinite=True`` reads the norm on the host
    and is refused while a stream is capturing."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    rng = _arena_grad_range(parameters) if float(norm_type) == 2.0 else None
    if rng is None:
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=norm_type,
                                              error_if_nonfinite=error_if_nonfinite, foreach=foreach)
    arena, s, e = rng
    C = _native.lib()
    g = arena.grad[s:e]
    part = torch.empty(C.grad_norm_parts(e - s), dtype=torch.float64, device=g.device)
    stats = torch.empty(3, dtype=torch.float32, device=g.device)
    C.grad_sumsq(g, part)
    if error_if_nonfinite:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("clip_grad_norm_(error_if_nonfinite=True) reads the norm on the host: "
                               "not possible while the stream is capturing")
        total = part.sum().sqrt().float()
        if not bool(torch.isfinite(total)):
            raise RuntimeError(
                f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be "
                "clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                "`error_if_nonfinite=False`")
    C.clip_scale(g, part, float(max_norm), stats)
    return stats[0]


def _arena_grad_range(parameters):
    """(arena, start, end) when the parameters with a gradient are GPU parameters of one arena, cover
    one gap-free run of it and each ``p.grad`` is its arena view; else None."""
    ps = [p for p in parameters if p.grad is not None]
    if not ps or _native.force_reference() or any(not p.is_cuda for p in ps):
        return None
    arena = getattr(ps[0], "_cdp_arena", None)
    if arena is None or arena.grad is None or any(getattr(p, "_cdp_arena", None) is not arena for p in ps):
        return None
    if len({id(p) for p in ps}) != len(ps) or arena.grad.dtype != torch.float32:
        return None
    base, es = arena.grad.data_ptr(), arena.grad.element_size()
    if any(p.grad.data_ptr() != base + arena.offsets[p._cdp_index] * es or p.grad.dtype != torch.float32 for p in ps):
        return None
    rng = arena.contiguous_range(ps)
    if rng is None or not _native.available():
        return None
    return arena, rng[0], rng[1]
