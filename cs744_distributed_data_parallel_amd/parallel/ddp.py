"""``DistributedDataParallel`` -- API-compatible wrapper on the native RCCL reducer.

Reference: ``model = DDP(model)`` at ``/root/reference/src/Part 3/main.py:61`` (torch's wrapper).
Behaviour kept:
  * construction: cross-rank parameter-shape verification, then parameters and buffers broadcast
    from rank 0 (here: ONE collective over the flat parameter arena + one over the buffer arena);
  * every training forward with ``broadcast_buffers=True`` re-broadcasts rank 0's buffers (BN
    running statistics) before running the module;
  * backward: bucketed all-reduce (average) overlapped with autograd via hooks; buckets are rebuilt
    in observed gradient-ready order after the first iteration;
  * ``.module``, ``module.``-prefixed ``state_dict``, ``no_sync()``, ``find_unused_parameters``
    (unused parameters raise unless enabled), ``bucket_cap_mb``.
MI355X specifics: gradients are arena views (zero-copy buckets), the averaging happens inside the
RCCL collective (ncclAvg), the all-reduce runs on the communicator's own stream, and
bucket caps default to xGMI-friendly sizes (:mod:`.buckets`).
"""
from __future__ import annotations

import contextlib
import hashlib
from typing import Optional

import torch
import torch.nn as nn

from ..utils.arena import BufferArena, arena_for, install_load_hooks
from .buckets import DEFAULT_BUCKET_CAP_MB, DEFAULT_FIRST_BUCKET_CAP_MB
from .comm import Communicator
from .reducer import GradReducer


def _tensors_in(obj, out):
    if isinstance(obj, torch.Tensor):
        out.append(obj)
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            _tensors_in(o, out)
    elif isinstance(obj, dict):
        for o in obj.values():
            _tensors_in(o, out)
    return out


class DistributedDataParallel(nn.Module):
    def __init__(
        self,
        module: nn.Module,
        device_ids=None,
        output_device=None,
        dim: int = 0,
        broadcast_buffers: bool = True,
        process_group=None,
        bucket_cap_mb: Optional[float] = None,
        find_unused_parameters: bool = False,
        check_reduction: bool = False,
        gradient_as_bucket_view: bool = True,
        static_graph: bool = False,
        first_bucket_cap_mb: Optional[float] = None,
        comm: Optional[Communicator] = None,
        rebuild_buckets: bool = True,
    ):
        super().__init__()
        self.module = module
        install_load_hooks(module)  # loaded weights refresh the optimizer's prepared products
        self.device_ids = device_ids
        self.broadcast_buffers = broadcast_buffers
        self.find_unused_parameters = find_unused_parameters
        self.require_backward_grad_sync = True
        self.require_forward_param_sync = True
        self.static_graph = static_graph
        params = [p for p in module.parameters() if p.requires_grad]
        if not params:
            raise RuntimeError("DistributedDataParallel is not needed when a module doesn't have any parameter "
                               "that requires a gradient.")
        if comm is None:
            from .. import distributed as D

            comm = D.communicator_for(params[0])
        self.comm = comm
        self.world_size = comm.size
        self._verify_shapes(params)
        self.arena = arena_for(params)
        bufs = [b for b in module.buffers() if b is not None]
        self._buffers_arena = BufferArena(bufs) if (bufs and broadcast_buffers) else None
        self._sync_module_states()
        self.reducer = GradReducer(
            self.arena,
            comm,
            bucket_cap_mb if bucket_cap_mb is not None else DEFAULT_BUCKET_CAP_MB,
            first_bucket_cap_mb if first_bucket_cap_mb is not None else DEFAULT_FIRST_BUCKET_CAP_MB,
            find_unused_parameters,
            average=True,
            # no explicit cap: the plan is designed at the ready-order rebuild from the measured
            # backward timeline and communicator (buckets.plan_buckets_timed)
            timed_plan=bucket_cap_mb is None and first_bucket_cap_mb is None and rebuild_buckets,
        )
        self._rebuild = rebuild_buckets
        self._rebuilt = False
        self._step_opt = None
        self._early_bcast = False

    def overlap_optimizer(self, optimizer):
        """Opt-in: run ``optimizer``'s step bucket by bucket inside backward, each bucket's SGD on the
        reducer's step stream right after that bucket's all-reduce (so it overlaps the remaining
        buckets' communication and backward compute, instead of following the last bucket on the
        compute stream). ``optimizer.step()`` then only completes the bookkeeping. Applies to
        iterations with gradient sync on the RCCL communicator once the buckets are rebuilt in ready
        order (before that, and under ``no_sync``, the step runs whole as usual). The result is
        bitwise the end-of-step SGD's. Needs this package's ``SGD`` over the module's parameters.

        Anything done to the gradients between ``backward()`` and ``step()`` (an in-place rescale,
        ``clip_grad_norm_``, ...) is not seen by an overlapped step: its SGD has already run inside
        backward. An ``SGD`` built with ``max_grad_norm`` or ``skip_nonfinite`` needs the norm of
        the whole model, so it declines the split and its step runs whole at ``step()``, after the
        last all-reduce. So does one built with ``ema_decay`` or ``lr_schedule``: the per-bucket
        launches carry neither the EMA nor the schedule (whose step index the last launch of a
        ``step()`` advances), so the step runs whole at ``step()``."""
        if not hasattr(optimizer, "bucket_steps"):
            raise TypeError("overlap_optimizer needs cs744_distributed_data_parallel_amd.SGD")
        self._step_opt = optimizer
        return self

    def early_buffer_broadcast(self, optimizer):
        """Opt-in (RCCL communicator, native reducer): broadcast rank 0's buffers (BatchNorm running
        statistics) at the end of every synced backward -- on the comm stream right behind the last
        gradient bucket -- instead of at the start of the next forward, where the compute stream
        waits for it. ``optimizer.step()`` (this package's ``SGD``) joins it afterwards, so the
        broadcast runs under the SGD; the next forward then skips its own broadcast.

        The buffers only change in forward, so forward k+1 sees the values torch DDP would
        broadcast to it -- unless rank 0's buffers are modified between backward k and forward k+1
        (e.g. a ``load_state_dict`` there), which then reaches the other ranks one step later.
        Returns self; a no-op without buffers to broadcast."""
        if not hasattr(optimizer, "add_post_step_join"):
            raise TypeError("early_buffer_broadcast needs cs744_distributed_data_parallel_amd.SGD")
        if self._buffers_arena is None or not self._bcast_needed():
            return self
        self.reducer.set_post_broadcast(list(self._buffers_arena.flats()))
        optimizer.add_post_step_join(self._join_early_broadcast)
        self._early_bcast = True
        return self

    def _join_early_broadcast(self):
        self.reducer.join_post_broadcast()

    def _bcast_needed(self):
        # one rank has nothing to broadcast -- except under the modelled-xGMI test mode, where the
        # one rank stands in for W and its collectives carry the modelled cost
        return self.world_size > 1 or getattr(self.comm, "models_world", 0) > 1

    def _register_bucket_steps(self):
        opt, red = self._step_opt, self.reducer
        red.set_bucket_steps(None)
        opt.cancel_bucket_steps()
        if not red.can_step_buckets():
            return
        steps = opt.bucket_steps(red.bucket_ranges, red)
        if steps is not None:
            red.set_bucket_steps(steps)

    # ------------------------------------------------------------------ construction-time sync
    def _verify_shapes(self, params):
        if self.world_size == 1:
            return
        sig = ";".join(f"{tuple(p.shape)}:{p.dtype}" for p in params).encode()
        h = int.from_bytes(hashlib.sha1(sig).digest()[:7], "little")
        dev = params[0].device
        t = torch.tensor([h, len(params)], dtype=torch.int64, device=dev)
        mx, mn = t.clone(), t.clone()
        self.comm.all_reduce(mx, "max")
        self.comm.all_reduce(mn, "min")
        if not torch.equal(mx, mn):
            raise RuntimeError("DistributedDataParallel: parameter shapes differ across ranks")

    @torch.no_grad()
    def _sync_module_states(self):
        if self.world_size == 1:
            return
        self.comm.broadcast(self.arena.data, 0)
        # a raw arena write bumps no parameter's _version: drop the optimizer's prepared weight
        # products (W^T, f16x2 maxima) so the next forward re-derives them from rank 0's weights
        if hasattr(self.arena, "prep_valid"):
            self.arena.prep_valid = None
        if self._buffers_arena is not None:
            for f in self._buffers_arena.flats():
                self.comm.broadcast(f, 0)

    @torch.no_grad()
    def _sync_buffers(self):
        if self._buffers_arena is None or not self._bcast_needed():
            return
        for f in self._buffers_arena.flats():
            self.comm.broadcast(f, 0)

    # ------------------------------------------------------------------ forward
    def forward(self, *inputs, **kwargs):
        grad_sync = torch.is_grad_enabled() and self.require_backward_grad_sync
        if grad_sync and self._rebuild and not self._rebuilt and self.reducer.iterations >= 1:
            self.reducer.rebuild_in_ready_order()
            self._rebuilt = True
        if grad_sync:
            self.reducer.rebind_if_stream_changed()
        # like torch DDP: the buffer broadcast of forward k is decided by forward k-1 (so the first
        # no-grad eval forward after training still syncs once)
        if self.broadcast_buffers and self.require_forward_param_sync:
            if self._early_bcast and self.reducer.take_post_issued() > 0:
                self._join_early_broadcast()  # the last backward broadcast them (usually joined already)
            else:
                self._sync_buffers()
        out = self.module(*inputs, **kwargs)
        if grad_sync:
            self.require_forward_param_sync = True
            self.reducer.prepare_for_backward(_tensors_in(out, []))
            if self._step_opt is not None:
                self._register_bucket_steps()
        else:
            self.require_forward_param_sync = False
        return out

    @contextlib.contextmanager
    def no_sync(self):
        """Accumulate gradients locally (no all-reduce) inside this context."""
        old = self.require_backward_grad_sync
        self.require_backward_grad_sync = False
        try:
            yield
        finally:
            self.require_backward_grad_sync = old

    # ------------------------------------------------------------------ misc API
    def bucket_sizes_bytes(self):
        return self.reducer.bucket_sizes_bytes()

    def _get_ddp_logging_data(self):
        return {
            "overlapped_step_buckets": self.reducer.stepped_buckets() if self._step_opt is not None else 0,
            "early_buffer_broadcast": self._early_bcast,
            "bucket_sizes": self.reducer.bucket_sizes_bytes(),
            "num_buckets": self.reducer.num_buckets,
            "native_reducer": self.reducer.native,
            "comm": getattr(self.comm, "kind", "?"),
            "world_size": self.world_size,
            "rebuilt_buckets": self._rebuilt,
        }

    def train(self, mode: bool = True):
        super().train(mode)
        return self
