"""Mirror of the reference `utils/custom_optims.py` (WeightDecay) plus the fused train-step tail.

* `WeightDecay`      -- same semantics as custom_optims.py:3-42: p -= (lr/base_lr) * weight_decay * p.
* `FusedClipAdamWWD` -- clip_grad_norm_(max_norm) + torch.optim.AdamW(weight_decay=0) + WeightDecay
  (train.py:163-165 / :170-172) as ONE pass over the model's flat fp32 buffers (rgbnm_clip_adamw_wd_step).
  The decayed set follows the reference's name filter (".weight" in name and "lrnorm" not in name,
  pipeline_utils.py:537).  `param_groups[0]['lr']` is honoured, so torch LR schedulers drive it unchanged.
  `state_dict()` / `load_state_dict()` carry the Adam moments and the step count in torch.optim.AdamW's own layout
  (state[i] = {step, exp_avg, exp_avg_sq} per parameter), so train.py's checkpoint / resume (train.py:195,
  pipeline_utils.py:490-580) works, and a checkpoint written by the reference's AdamW loads here (and vice versa).
* `DeviceLossScaler` -- torch.amp.GradScaler(1.6, 0.625, 600) + pipeline_utils.clip_gradscaler (train.py:160-167,
  pipeline_utils.py:399-409, 541) with the scale, the inf / NaN check, the skipped step and the scale update on the device,
  inside FusedClipAdamWWD's two launches (rgbnm_clip_adamw_wd_step_scaled): fp16 training without a host sync.
* `DeviceLRSchedule` -- train.py's warm-up + cosine learning-rate schedule (train.py:149-152, 174-176, pipeline_utils.py:538) as
  a float64 table on the device, looked up inside the same two launches (rgbnm_clip_adamw_wd_step_sched) once it is attached
  with FusedClipAdamWWD.attach_schedule: no argument of the step changes between steps, so the step can be captured.
"""
import math

import torch
from torch.optim.optimizer import Optimizer

from . import lib as L


class WeightDecay(Optimizer):
    """Additive, schedule-relative weight decay (reference: utils/custom_optims.py:3-42)."""

    def __init__(self, params, lr: float = 1e-3, weight_decay: float = 0.0):
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        super().__init__(params, dict(lr=lr, base_lr=lr, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            f = -((group["lr"] / group["base_lr"]) * group["weight_decay"])
            ps = [p for p in group["params"]]
            if ps:
                torch._foreach_add_(ps, ps, alpha=f)


class FusedClipAdamWWD(Optimizer):
    def __init__(self, model, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=1.0):
        m = model.module if hasattr(model, "module") else model
        super().__init__(list(m.parameters()), dict(lr=lr, base_lr=lr, betas=betas, eps=eps,
                                                    weight_decay=weight_decay, max_norm=max_norm))
        self._m = m
        self._step = 0
        self._dev_step = None          # the DeviceLossScaler whose state block holds the step count while it is the truth
        self._state_ready = False
        self.last_norm = None
        self._sched = None             # the attached DeviceLRSchedule
        self._neutral = None           # the scale-1 DeviceLossScaler an attached schedule steps under when no scaler is given

    def attach_schedule(self, schedule):
        """From now on step() and step(loss_scaler=...) take lr and wd_factor from `schedule`'s device table
        (rgbnm_clip_adamw_wd_step_sched) and do not read param_groups[0]['lr']; base_lr and weight_decay stay the group's.
        Every upload happens here or on the first step after it (the table, the state blocks, the Adam step count); later
        steps neither sync nor upload, so a step() under torch.cuda.graph capture succeeds and replays.
        The entry always runs under a loss-scale block.  With no DeviceLossScaler (bf16 / fp32 training) the optimizer passes a
        neutral one of its own (scale 1, both factors 1, scale_min = scale_max = 1): the arithmetic of the plain step on
        gradients multiplied by 1.0f, with ONE visible consequence -- a non-finite gradient norm skips the step and counts in
        skipped_steps(), where the plain step() would write NaN into the weights.  state_dict() and the read-back of the step
        count behave as under a DeviceLossScaler."""
        if not isinstance(schedule, DeviceLRSchedule):
            raise TypeError(f"attach_schedule needs a DeviceLRSchedule, got {type(schedule).__name__}")
        self._ensure()
        dev = self._m._flat.device
        schedule._device(dev)
        if self._neutral is None:
            self._neutral = DeviceLossScaler(init_scale=1.0, growth_factor=1.0, backoff_factor=1.0, scale_min=1.0, scale_max=1.0)
        self._neutral._device_state(dev)
        self._sched = schedule

    def detach_schedule(self):
        """Back to param_groups[0]['lr'] (the host scheduler's); the schedule keeps its position."""
        self._sched = None
        if self._dev_step is not None and self._dev_step is self._neutral:
            self._read_back_step()

    def skipped_steps(self):
        """Steps the neutral loss-scale block skipped because the gradient norm was not finite (syncs; logging only).  Steps
        under a DeviceLossScaler count in that scaler."""
        return self._neutral.skipped_steps() if self._neutral is not None else 0

    def _ensure(self):
        m = self._m
        m._ensure_flat()
        if not self._state_ready or self._exp_avg.numel() != m._flat.numel() or self._exp_avg.device != m._flat.device:
            self._exp_avg = torch.zeros_like(m._flat)
            self._exp_avg_sq = torch.zeros_like(m._flat)
            self._ws = torch.empty(max(L.lib().rgbnm_clip_adamw_wd_workspace(), L.lib().rgbnm_clip_adamw_wd_scaled_workspace(),
                                       L.lib().rgbnm_clip_adamw_wd_sched_workspace()), device=m._flat.device, dtype=torch.uint8)
            self._norm = torch.zeros(1, device=m._flat.device, dtype=torch.float32)
            self._gather = None
            self._state_ready = True
            self._publish_state()

    def _publish_state(self):
        """Expose the flat moment buffers as torch.optim.AdamW-style per-parameter state (views, always current)."""
        m = self._m
        self.state.clear()
        for n, p in m._named.items():
            self.state[p] = {"step": torch.tensor(float(self._step)), "exp_avg": m._gview(self._exp_avg, n),
                             "exp_avg_sq": m._gview(self._exp_avg_sq, n)}

    def _read_back_step(self):
        """After steps under a DeviceLossScaler the step count lives on the device (skipped steps do not count): fetch it.
        The one host sync of that mode; state_dict() and the first plain step() after it come through here."""
        if self._dev_step is not None:
            self._step = self._dev_step._device_step()
            if self._sched is None:    # (with a schedule attached the block stays the truth: a captured step goes on counting there)
                self._dev_step = None

    def _hand_step_to(self, s):
        """Make DeviceLossScaler `s`'s state block the holder of the Adam step count (syncs if another block held it, uploads)."""
        self._read_back_step()                         # (another scaler's count, if there was one)
        s._set_device_step(self._step)
        self._dev_step = s

    def state_dict(self):
        self._ensure()
        self._read_back_step()
        for st in self.state.values():
            st["step"] = torch.tensor(float(self._step))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Restore moments + step (written by this class or by torch.optim.AdamW over the same parameter list)."""
        self._ensure()
        own = [dict((k, v) for k, v in g.items() if k != "params") for g in self.param_groups]
        super().load_state_dict(state_dict)          # validates groups / sizes, casts to the parameter devices
        for g, o in zip(self.param_groups, own):
            if "base_lr" not in g:                   # a torch.optim.AdamW checkpoint: its weight_decay (0, the decay lives
                g["weight_decay"] = o["weight_decay"]     # in the reference's separate WeightDecay optimizer) is not ours
            for k, v in o.items():
                g.setdefault(k, v)                   # base_lr, max_norm, ... keep this optimizer's values
        m = self._m
        steps = set()
        loaded = dict(self.state)
        for n, p in m._named.items():
            st = loaded.get(p)
            if not st:                               # parameter without state (never stepped): zero moments
                m._gview(self._exp_avg, n).zero_()
                m._gview(self._exp_avg_sq, n).zero_()
                continue
            m._gview(self._exp_avg, n).copy_(st["exp_avg"])
            m._gview(self._exp_avg_sq, n).copy_(st["exp_avg_sq"])
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"FusedClipAdamWWD keeps ONE step count for all parameters; the state has {sorted(steps)}")
        self._step = steps.pop() if steps else 0
        if self._sched is not None and self._dev_step is not None:
            self._dev_step._set_device_step(self._step)     # a captured step cannot upload it later: the block gets it now
        else:
            self._dev_step = None                    # the loaded count is the truth; the next scaled step uploads it
        self._publish_state()

    def _flat_grads(self):
        """The flat fp32 gradient buffer: zero-copy when every .grad is the view the backward kernels wrote (the
        normal case, also after DDP's in-place all-reduce), otherwise gathered into a staging buffer."""
        m = self._m
        base = m.flat_grad_base()
        if base is not None:
            return base
        if self._gather is None:
            self._gather = torch.zeros_like(m._flat)
        views, grads = [], []
        for n, p in m._named.items():
            if p.grad is None:
                raise L.RgbnmError(f"parameter {n} has no gradient")
            views.append(m._gview(self._gather, n))
            grads.append(p.grad)
        torch._foreach_copy_(views, grads)
        return self._gather.data_ptr()

    @torch.no_grad()
    def step(self, loss_scaler=None):
        """One fused step.  loss_scaler: a DeviceLossScaler (call it through loss_scaler.step(optimizer), as train.py calls
        gradscaler.step): the gradients carry its scale; they are unscaled, checked, and the step is taken or skipped on the
        device, where the scale is updated too.  The Adam step count then lives in the scaler's state block (initialised from
        the host count on first use; state_dict() reads it back, the only sync; a later plain step() reads it back once
        first), and last_norm is the norm of the UNSCALED gradients (non-finite on a skipped step).
        FlatGradSync.wait() stays in front: the gradients are final, and the same on every rank, before the check runs, and
        the all-reduced sum of a non-finite gradient is non-finite on every rank, so all ranks skip together."""
        self._ensure()
        g = self.param_groups[0]
        m = self._m
        if loss_scaler is not None and not loss_scaler._enabled:
            loss_scaler = None
        if self._sched is not None:
            return self._step_sched(loss_scaler)
        if loss_scaler is None:
            self._read_back_step()
            self._step += 1
        if m._grad_sync is not None:       # overlapped flat all-reduce (parallel.FlatGradSync): gradients are final after this
            m._grad_sync.wait()
        gptr = self._flat_grads()
        wd_factor = (g["lr"] / g["base_lr"]) * g["weight_decay"]
        max_norm = g["max_norm"] if g["max_norm"] else 0.0
        if loss_scaler is None:
            L.check(L.lib().rgbnm_clip_adamw_wd_step(
                m._flat.data_ptr(), gptr, self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr(),
                m._wd_flags.data_ptr(), m._flat.numel(), g["lr"], g["betas"][0], g["betas"][1], g["eps"], self._step,
                wd_factor, max_norm, self._norm.data_ptr(), self._ws.data_ptr(), self._ws.numel(), L.stream()),
                "clip_adamw_wd_step")
        else:
            s = loss_scaler
            state = s._device_state(m._flat.device)
            if self._dev_step is not s:
                self._hand_step_to(s)
            L.check(L.lib().rgbnm_clip_adamw_wd_step_scaled(
                m._flat.data_ptr(), gptr, self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr(),
                m._wd_flags.data_ptr(), m._flat.numel(), g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                wd_factor, max_norm, self._norm.data_ptr(), state.data_ptr(), s._growth_factor, s._backoff_factor,
                s._growth_interval, s._scale_min, s._scale_max, self._ws.data_ptr(), self._ws.numel(), L.stream()),
                "clip_adamw_wd_step_scaled")
        self.last_norm = self._norm

    def _prepare_sched(self, loss_scaler=None):
        """The loss-scale block an attached schedule steps under (loss_scaler's, or the neutral one), holding the Adam step
        count.  Uploads and syncs on first use only; that first use cannot be a captured one."""
        s = loss_scaler if loss_scaler is not None and loss_scaler._enabled else self._neutral
        if s._state is None or self._dev_step is not s:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the first step() with an attached schedule (or after a change of loss scaler) uploads the "
                                   "Adam step count and cannot be captured: take one eager step first")
            s._device_state(self._m._flat.device)
            self._hand_step_to(s)
        return s

    def _step_sched(self, loss_scaler):
        m, g = self._m, self.param_groups[0]
        s = self._prepare_sched(loss_scaler)
        if m._grad_sync is not None:
            m._grad_sync.wait()
        gptr = self._flat_grads()
        sch = self._sched
        L.check(L.lib().rgbnm_clip_adamw_wd_step_sched(
            m._flat.data_ptr(), gptr, self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr(), m._wd_flags.data_ptr(),
            m._flat.numel(), sch._table.data_ptr(), sch._table.numel(), g["base_lr"], g["weight_decay"], g["betas"][0],
            g["betas"][1], g["eps"], g["max_norm"] if g["max_norm"] else 0.0, self._norm.data_ptr(), s._state.data_ptr(),
            sch._state.data_ptr(), s._growth_factor, s._backoff_factor, s._growth_interval, s._scale_min, s._scale_max,
            self._ws.data_ptr(), self._ws.numel(), L.stream()), "clip_adamw_wd_step_sched")
        self.last_norm = self._norm


class DeviceLRSchedule:
    """A learning-rate schedule as a float64 table on the device: entry k is what param_groups[0]['lr'] holds at the
    optimizer.step() of iteration k under the host scheduler the table was recorded from.  FusedClipAdamWWD.attach_schedule
    makes the fused tail look it up (include/rgbnm.h, rgbnm_lr_sched_state: the block counts every call, skipped steps included,
    as train.py steps its scheduler every iteration); past the last entry the last entry holds.  train.py:149-152, 174-176

        if current_itr < WARMUP: adjust_lr(optimizer, LR * (current_itr + 1) / WARMUP); copy_lr(optimizer, weight_decayer)
        ...
        if current_itr >= WARMUP: cosinescheduler.step(); copy_lr(optimizer, weight_decayer)

    become `optimizer.attach_schedule(DeviceLRSchedule.warmup_cosine(LR, WARMUP, max_iters))`, once, before the loop.
    get_last_lr(), iteration() and state_dict() sync; they are for logging and checkpoints."""

    def __init__(self, values):
        t = torch.tensor([float(x) for x in values], dtype=torch.float64)
        if t.numel() < 1:
            raise ValueError("a DeviceLRSchedule needs at least one learning rate")
        if not bool(torch.isfinite(t).all()) or bool((t < 0).any()):
            raise ValueError("learning rates must be finite and not negative")
        self._values = t
        self._iter = 0              # until the state block exists
        self._table = None          # float64 [len] on the device
        self._state = None          # int32 [8] on the device: rgbnm_lr_sched_state

    @classmethod
    def from_scheduler(cls, make_scheduler, n_iters, base_lr, warmup=0):
        """Record n_iters iterations of train.py's loop (train.py:149-152, 174-176) run on the host against a dummy AdamW of
        learning rate base_lr and the torch scheduler `make_scheduler(optimizer)` returns.  The doubles stored are the ones
        torch's scheduler leaves in param_groups[0]['lr'] (its own recursion), not a closed form.  As in train.py, current_itr
        is incremented before it is compared: iteration k runs with current_itr = k + 1."""
        opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=base_lr, weight_decay=0)
        sched = make_scheduler(opt)
        values, current_itr = [], 0
        for _ in range(int(n_iters)):
            current_itr += 1
            if current_itr < warmup:
                for g in opt.param_groups:
                    g["lr"] = base_lr * (current_itr + 1) / warmup
            values.append(opt.param_groups[0]["lr"])
            opt.step()
            if current_itr >= warmup:
                sched.step()
        return cls(values)

    @classmethod
    def warmup_cosine(cls, base_lr, warmup, max_iters):
        """The reference's schedule: linear warm-up, then CosineAnnealingLR(T_max = max_iters - warmup, eta_min = 0)
        stepped every iteration (pipeline_utils.py:538)."""
        return cls.from_scheduler(
            lambda opt: torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=max_iters - warmup, eta_min=0), max_iters, base_lr,
            warmup)

    def __len__(self):
        return self._values.numel()

    def values(self):
        """The table as Python floats (the host copy)."""
        return self._values.tolist()

    def _device(self, device):
        if self._state is None:
            self._table = self._values.to(device)
            st = torch.zeros(8, dtype=torch.int32)
            st[0] = self._iter
            self._state = st.to(device)
        return self._state

    def iteration(self):
        """Calls seen so far, skipped steps included (syncs)."""
        if self._state is not None:
            self._iter = int(self._state[0].item())
        return self._iter

    def get_last_lr(self):
        """[lr of the latest step] as torch schedulers report it, in full precision (syncs); before the first step, entry 0."""
        k = min(max(self.iteration() - 1, 0), len(self) - 1)
        return [float(self._values[k])]

    def state_dict(self):
        return {"iter": self.iteration(), "table_len": len(self)}

    def load_state_dict(self, state_dict):
        if int(state_dict["table_len"]) != len(self):
            raise ValueError(f"the schedule state belongs to a table of {state_dict['table_len']} entries, this one has {len(self)}")
        self._iter = int(state_dict["iter"])
        if self._state is not None:
            self._state[:1].fill_(self._iter)


class DeviceLossScaler:
    """torch.amp.GradScaler for FusedClipAdamWWD with everything on the device.  The defaults are the reference's:
    GradScaler(growth 1.6, backoff 0.625, interval 600) (utils/configs.py:37-40, pipeline_utils.py:541), clamped after every
    update to [2^-4, 2^18] (clip_gradscaler, pipeline_utils.py:399-409).  train.py:160-167 becomes

        scaler.scale(loss).backward()
        scaler.step(optimizer)          # unscale_ + clip_grad_norm_ + both optimizer steps + update + clip_gradscaler
        scaler.update()                 # no-op, kept for the loop's shape

    with no host sync: scale() multiplies by a device scalar that aliases the state block's scale, the fused tail reads and
    updates the block (include/rgbnm.h, rgbnm_loss_scale_state).  get_scale(), skipped_steps() and state_dict() sync; they
    are for logging and checkpoints.  state_dict() has torch.amp.GradScaler's keys, so a scaler state written by the
    reference's checkpoint (pipeline_utils.py:490-516) loads here and the reverse.  Before the first device use the state is
    held on the host (as GradScaler holds its init_scale)."""

    def __init__(self, init_scale=2.0 ** 16, growth_factor=1.6, backoff_factor=0.625, growth_interval=600,
                 scale_min=2.0 ** -4, scale_max=2.0 ** 18, enabled=True):
        if enabled:
            if not growth_factor > 0.0 or not backoff_factor > 0.0:
                raise ValueError("growth_factor and backoff_factor must be positive")
            if int(growth_interval) < 1:
                raise ValueError("growth_interval must be at least 1")
            if not scale_min <= scale_max:
                raise ValueError("scale_min must not exceed scale_max")
        self._enabled = bool(enabled)
        self._growth_factor, self._backoff_factor = float(growth_factor), float(backoff_factor)
        self._growth_interval = int(growth_interval)
        self._scale_min, self._scale_max = float(scale_min), float(scale_max)
        self._host = {"scale": float(init_scale), "_growth_tracker": 0}     # until the state block exists
        self._state = None          # int32 [8] on the device: rgbnm_loss_scale_state
        self._scale_t = None        # 0-dim fp32 view of its first word

    def is_enabled(self):
        return self._enabled

    def _device_state(self, device):
        if self._state is None:
            st = torch.zeros(8, dtype=torch.int32)
            st[:1].view(torch.float32)[0] = self._host["scale"]
            st[1] = self._host["_growth_tracker"]
            st[3] = self._host.get("skipped", 0)
            self._state = st.to(device)
            self._scale_t = self._state[:1].view(torch.float32)[0]
        return self._state

    def _pull(self):
        """Device state -> host copy (syncs)."""
        if self._state is not None:
            st = self._state.cpu()
            self._host = {"scale": float(st[:1].view(torch.float32)[0]), "_growth_tracker": int(st[1]), "skipped": int(st[3])}
        return self._host

    def _device_step(self):
        return int(self._state[2].item())

    def _set_device_step(self, step):
        self._state[2:3].fill_(int(step))

    def scale(self, loss):
        if not self._enabled:
            return loss
        self._device_state(loss.device)
        return loss * self._scale_t

    def step(self, optimizer):
        if not isinstance(optimizer, FusedClipAdamWWD):
            raise TypeError(f"DeviceLossScaler.step needs a FusedClipAdamWWD (the scaler lives in its fused tail), got "
                            f"{type(optimizer).__name__}")
        if not self._enabled:
            return optimizer.step()
        return optimizer.step(loss_scaler=self)

    def update(self):
        """Nothing to do: the scale was updated (and clamped) on the device inside step().  Kept so that the loop keeps
        train.py's shape."""

    def get_scale(self):
        """The current scale as a float (syncs; logging only)."""
        return self._pull()["scale"] if self._enabled else 1.0

    def skipped_steps(self):
        """Steps skipped so far because a gradient was not finite (syncs; logging only)."""
        return self._pull().get("skipped", 0) if self._enabled else 0

    def state_dict(self):
        if not self._enabled:
            return {}
        h = self._pull()
        return {"scale": h["scale"], "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": h["_growth_tracker"]}

    def load_state_dict(self, state_dict):
        if not self._enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled scaler.")
        self._growth_factor, self._backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._host = {"scale": float(state_dict["scale"]), "_growth_tracker": int(state_dict["_growth_tracker"]),
                      "skipped": self._pull().get("skipped", 0)}
        if self._state is not None:
            st = torch.zeros(2, dtype=torch.int32)
            st[:1].view(torch.float32)[0] = self._host["scale"]
            st[1] = self._host["_growth_tracker"]
            self._state[:2].copy_(st)
