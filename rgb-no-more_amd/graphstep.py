"""The whole train step as ONE HIP graph: forward -> loss -> (loss scale) -> backward -> fused optimizer tail.

bench.py replays mixup-out -> forward -> loss -> backward and leaves the optimizer eager, because its two launches took lr,
wd_factor and the step count by value.  With the schedule on the device (custom_optims.DeviceLRSchedule, include/rgbnm.h
rgbnm_clip_adamw_wd_step_sched) no argument of the step changes between steps, so train.py:146-176

    optimizer.zero_grad(); warm-up lr; forward; loss; scale(loss).backward(); unscale_, clip, step, step, update; scheduler.step()

becomes

    step = CapturedTrainStep(model, optimizer, DeviceLRSchedule.warmup_cosine(LR, WARMUP, max_iters), loss_scaler)
    step.capture(y, cbcr, target)            # static tensors (or LazyMixed / LazyTarget around static buffers), once
    for batch in loader:
        refresh y, cbcr, target in place     # the data stage writes the static buffers
        loss = step.replay()                 # one graph launch; `loss` is the static loss tensor

The data stage (sampling, augment, mixup) stays outside: its parameters are drawn on the host.  A gradient exchange (world > 1)
sits between backward and tail and is not captured: such a run keeps its eager loop and can still attach the schedule."""
import torch

from . import cls_transforms
from .custom_optims import DeviceLossScaler, DeviceLRSchedule, FusedClipAdamWWD

WARMUP_PASSES = 2           # eager forward + backward passes before the capture, as bench.py runs them


class CapturedTrainStep:
    def __init__(self, model, optimizer, schedule, loss_scaler=None, criterion=cls_transforms.cross_entropy):
        m = model.module if hasattr(model, "module") else model
        if not isinstance(optimizer, FusedClipAdamWWD):
            raise TypeError(f"CapturedTrainStep needs a FusedClipAdamWWD, got {type(optimizer).__name__}")
        if not isinstance(schedule, DeviceLRSchedule):
            raise TypeError(f"CapturedTrainStep needs a DeviceLRSchedule, got {type(schedule).__name__}")
        if loss_scaler is not None and not isinstance(loss_scaler, DeviceLossScaler):
            raise TypeError("loss_scaler must be a DeviceLossScaler (a host GradScaler syncs in step())")
        if getattr(m, "_grad_sync", None) is not None:
            raise RuntimeError("the model has a gradient exchange attached (_grad_sync): it runs between backward and optimizer "
                               "tail and cannot be captured.  Keep the eager loop; optimizer.attach_schedule() works there too")
        if getattr(m, "train_dropout", False):
            raise RuntimeError("train_dropout = True: that a replay draws fresh dropout masks (as SwinV2's DropPath does) has not "
                               "been shown for the in-kernel Philox masks, so capture is refused.  Keep the eager loop; "
                               "optimizer.attach_schedule() works there too")
        if loss_scaler is not None and not loss_scaler.is_enabled():
            loss_scaler = None
        self.model, self._m, self.optimizer, self.schedule, self.loss_scaler = model, m, optimizer, schedule, loss_scaler
        self.criterion = criterion
        self.graph = None
        self.loss = None            # the static loss tensor of the captured pass
        self.logits = None          # ... and its logits

    def _drop_path_active(self):
        return self._m.training and any(getattr(b, "drop_path_p", 0.0) > 0.0 for b in self._m.modules())

    def _compute_dtype(self):
        cdt = getattr(self._m, "compute_dtype", None)
        if cdt is None:
            cdt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else torch.float32
        return cdt

    def _forward_backward(self, inputs, cdt):
        y, cbcr, target = inputs
        logits = self.model(y, cbcr)
        loss = self.criterion(logits, target, grad_dtype=cdt)
        (self.loss_scaler.scale(loss) if self.loss_scaler is not None else loss).backward()
        return loss, logits

    def _tail(self):
        if self.loss_scaler is not None:
            self.loss_scaler.step(self.optimizer)
            self.loss_scaler.update()
        else:
            self.optimizer.step()

    def _blocks(self):
        """Everything a step writes besides the activations: weights, moments, norm, both state blocks."""
        o = self.optimizer
        s = o._prepare_sched(self.loss_scaler)
        return [self._m._flat, o._exp_avg, o._exp_avg_sq, o._norm, s._state, self.schedule._state]

    def capture(self, y, cbcr, target):
        """Warm up eagerly, capture, and check one replay against one eager step bit for bit on the flat weights (both moment
        buffers and the loss too); weights, moments and both state blocks are then back where they were, so the first
        replay() is step 1.  With DropPath active (SwinV2, drop_path_rate > 0, train mode) the masks advance with the replays as
        bench.py notes, so the replay is held to a finite loss only: capture with drop_path_rate = 0 to check the bits.
        Must run on a non-default stream (torch.cuda.stream(...)): the legacy default stream cannot be captured."""
        if self.graph is not None:
            raise RuntimeError("already captured")
        stream = torch.cuda.current_stream()
        if stream == torch.cuda.default_stream():
            raise RuntimeError("capture() must run on a non-default stream: `with torch.cuda.stream(torch.cuda.Stream()):`")
        o, inputs = self.optimizer, (y, cbcr, target)
        if o._sched is not self.schedule:
            o.attach_schedule(self.schedule)
        cdt = self._compute_dtype()
        blocks = self._blocks()                       # (creates the state blocks and uploads the Adam step count: eager)
        saved = [b.clone() for b in blocks]

        def restore():
            for b, s in zip(blocks, saved):
                b.copy_(s)

        # one eager step: the reference of the check below, and the tail's own warm-up
        o.zero_grad(set_to_none=True)
        loss, _ = self._forward_backward(inputs, cdt)
        self._tail()
        want = [b.clone() for b in blocks[:3]] + [loss.detach().clone()]
        restore()
        for _ in range(WARMUP_PASSES):                # the optimizer is not part of these
            o.zero_grad(set_to_none=True)
            self._forward_backward(inputs, cdt)
        o.zero_grad(set_to_none=True)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            self.loss, self.logits = self._forward_backward(inputs, cdt)
            self._tail()
        g.replay()
        torch.cuda.synchronize()
        got = blocks[:3] + [self.loss.detach()]
        equal = [torch.equal(a, b) for a, b in zip(got, want)]
        ok = bool(torch.isfinite(self.loss.detach()).all()) if self._drop_path_active() else all(equal)
        restore()
        torch.cuda.synchronize()
        if not ok:
            raise RuntimeError("graph replay of the train step does not reproduce the eager step bit for bit "
                               f"(weights, exp_avg, exp_avg_sq, loss equal: {equal})")
        self.graph = g
        return self

    def replay(self):
        """One train step on whatever the static inputs hold now.  Returns the static loss tensor (no sync)."""
        if self.graph is None:
            raise RuntimeError("capture() first")
        self.graph.replay()
        return self.loss
