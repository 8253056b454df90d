"""CPU checks of the device learning-rate schedule: the C ABI of rgbnm_clip_adamw_wd_step_sched (declared, exported, header and
binding agree, ABI version still 3, every host-side refusal returns before anything touches the device), and the tables
DeviceLRSchedule records -- float64 bit for bit against a literal host loop over train.py:146-176 with torch's own schedulers."""
import ctypes
import os
import re
import struct

import pytest
import torch

from rgb_no_more_amd import custom_optims as CO
from rgb_no_more_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -3
CTYPE = {"float*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "const unsigned char*": ctypes.c_void_p,
         "const double*": ctypes.c_void_p, "rgbnm_loss_scale_state*": ctypes.c_void_p, "rgbnm_lr_sched_state*": ctypes.c_void_p,
         "void*": ctypes.c_void_p, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double,
         "int": ctypes.c_int, "size_t": ctypes.c_size_t}


def bits(values):
    return [struct.pack("<d", float(v)) for v in values]


def header():
    txt = open(os.path.join(ROOT, "include", "rgbnm.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def header_args(name):
    m = re.search(r"\b(\w[\w ]*?)\s+" + name + r"\s*\(([^)]*)\)\s*;", header())
    assert m, name
    args = []
    for a in m.group(2).split(","):
        a = " ".join(a.split())
        if a == "void":
            continue
        args.append(re.sub(r"\s*\b\w+$", "", a).replace(" *", "*"))
    return m.group(1).strip(), args


def test_symbols_header_and_binding_agree():
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in ("rgbnm_clip_adamw_wd_step_sched", "rgbnm_clip_adamw_wd_sched_workspace"):
        assert hasattr(dll, name), name
        ret, args = header_args(name)
        res, argtypes = L.PROTOTYPES[name]
        assert res is CTYPE[ret], (name, ret)
        assert [CTYPE[a] for a in args] == argtypes, (name, args)
    # the scaled entry's arguments with (lr, wd_factor) replaced by the table and its two constants, and sched behind state
    _, old = header_args("rgbnm_clip_adamw_wd_step_scaled")
    _, new = header_args("rgbnm_clip_adamw_wd_step_sched")
    assert old[6] == "float" and old[10] == "float" and old[13] == "rgbnm_loss_scale_state*"
    assert new == (old[:6] + ["const double*", "int", "double", "double"] + old[7:10] + old[11:14] + ["rgbnm_lr_sched_state*"]
                   + old[14:])
    assert L.lib().rgbnm_abi_version() == 3 and L.ABI_VERSION == 3
    assert re.search(r"#define\s+RGBNM_ABI_VERSION\s+3\b", header())
    ws = L.lib().rgbnm_clip_adamw_wd_sched_workspace()
    assert ws >= L.lib().rgbnm_clip_adamw_wd_scaled_workspace() + 12 and ws % 4 == 0        # ... then lr, wd_factor, iter
    m = re.search(r"typedef struct rgbnm_lr_sched_state \{(.*?)\} rgbnm_lr_sched_state;", header(), flags=re.S)
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int iter", "float lr", "float wd_factor", "int reserved[5]"]
    # the loss-scale block is as it was
    m = re.search(r"typedef struct rgbnm_loss_scale_state \{(.*?)\} rgbnm_loss_scale_state;", header(), flags=re.S)
    assert [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()][5:] == ["int reserved[3]"]


def test_refusals_return_before_any_device_call():
    lib = L.lib()
    wsb = lib.rgbnm_clip_adamw_wd_sched_workspace()
    ok = dict(p=0x1000, g=0x2000, m=0x3000, v=0x4000, fl=0x5000, n=512, table=0x8000, tlen=8, base_lr=1e-3, wd=0.05, norm=None,
              state=0x6000, sched=0x9000, growth=1.6, backoff=0.625, interval=600, smin=2.0 ** -4, smax=2.0 ** 18, ws=0x7000, wsb=wsb)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.rgbnm_clip_adamw_wd_step_sched(a["p"], a["g"], a["m"], a["v"], a["fl"], a["n"], a["table"], a["tlen"], a["base_lr"],
                                                  a["wd"], 0.9, 0.999, 1e-8, 1.0, a["norm"], a["state"], a["sched"], a["growth"],
                                                  a["backoff"], a["interval"], a["smin"], a["smax"], a["ws"], a["wsb"], None)
    for k in ("p", "g", "m", "v", "fl", "state", "ws", "table", "sched"):
        assert call(**{k: None}) == EINVAL, k
    for n in (500, 0, -256, 257):
        assert call(n=n) == EINVAL, n
    for tlen in (0, -1):
        assert call(tlen=tlen) == EINVAL, tlen
    for b in (0.0, -1e-3, float("nan")):
        assert call(base_lr=b) == EINVAL, b
    for w in (-0.05, float("nan")):
        assert call(wd=w) == EINVAL, w
    for wsb_ in (0, 1024, lib.rgbnm_clip_adamw_wd_scaled_workspace(), wsb - 4):
        assert call(wsb=wsb_) == EWORKSPACE, wsb_
    for interval in (0, -1):
        assert call(interval=interval) == EINVAL, interval
    for f in (0.0, -1.6, float("nan")):
        assert call(growth=f) == EINVAL and call(backoff=f) == EINVAL, f
    assert call(smin=2.0, smax=1.0) == EINVAL and call(smin=float("nan")) == EINVAL
    assert call(table=None, wsb=0) == EINVAL            # arguments are checked first


# ------------------------------------------------------------------------------------------------------------ the tables
def train_py_lrs(base_lr, warmup, n_iters, make_scheduler):
    """train.py:146-176 on a dummy parameter: the lr of param_groups[0] at every optimizer.step()."""
    optimizer = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(3))], lr=base_lr, weight_decay=0, eps=1e-8)
    scheduler = make_scheduler(optimizer)
    current_itr, seen = 0, []
    for _ in range(n_iters):
        optimizer.zero_grad()
        current_itr += 1
        if current_itr < warmup:                                     # train.py:150-152 (adjust_lr)
            for g in optimizer.param_groups:
                g["lr"] = base_lr * (current_itr + 1) / warmup
        seen.append(optimizer.param_groups[0]["lr"])
        optimizer.step()                                             # train.py:164 / 171
        if current_itr >= warmup:                                    # train.py:174-176
            scheduler.step()
    return seen


def test_warmup_cosine_is_the_host_loop_bit_for_bit():
    want = train_py_lrs(3e-3, 5, 40, lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=40 - 5, eta_min=0))
    s = CO.DeviceLRSchedule.warmup_cosine(3e-3, 5, 40)
    assert len(s) == 40 and bits(s.values()) == bits(want)
    # the shape of it: train.py's warm-up starts at 2/5 (current_itr is incremented first), reaches base_lr, then falls
    assert want[0] == 3e-3 * 2 / 5 and want[3] == 3e-3 * 5 / 5 == want[4] and want[5] < want[4]
    assert all(a > b for a, b in zip(want[4:], want[5:])) and want[-2] > want[-1] == 0.0
    # and it is torch's recursion, not the closed form: the two differ in the last bits somewhere along the way
    import math
    closed = [want[4] * (1 + math.cos(math.pi * (k - 4) / 35)) / 2 for k in range(4, 40)]
    assert bits(closed) != bits(want[4:])
    assert max(abs(a - b) for a, b in zip(closed, want[4:])) < 1e-15


def test_from_scheduler_step_lr():
    make = lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=3, gamma=0.3)      # noqa: E731
    want = train_py_lrs(0.1, 0, 12, make)
    s = CO.DeviceLRSchedule.from_scheduler(make, 12, 0.1)
    assert bits(s.values()) == bits(want)
    assert want[0] == 0.1 and want[3] == 0.1 * 0.3 and len(set(want)) == 4
    assert s.get_last_lr() == [0.1] and s.iteration() == 0


def test_the_table_the_captured_step_tests_use_ends_at_zero():
    v = CO.DeviceLRSchedule.warmup_cosine(1e-3, 3, 6).values()
    assert v[0] == 1e-3 * 2 / 3 and v[1] == 1e-3 * 3 / 3 == v[2] and v[2] > v[3] > v[4] > v[5] == 0.0


def test_state_dict_round_trip_and_length_mismatch():
    s = CO.DeviceLRSchedule([0.1, 0.05, 0.0])
    assert s.state_dict() == {"iter": 0, "table_len": 3}
    s.load_state_dict({"iter": 2, "table_len": 3})
    assert s.iteration() == 2 and s.state_dict() == {"iter": 2, "table_len": 3} and s.get_last_lr() == [0.05]
    t = CO.DeviceLRSchedule([0.1, 0.05, 0.0])
    t.load_state_dict(s.state_dict())
    assert t.state_dict() == s.state_dict()
    t.load_state_dict({"iter": 7, "table_len": 3})          # past the end: the last entry holds
    assert t.get_last_lr() == [0.0]
    with pytest.raises(ValueError):
        CO.DeviceLRSchedule([0.1, 0.05]).load_state_dict(s.state_dict())
    for bad in ([], [float("nan")], [-1e-3], [float("inf")]):
        with pytest.raises(ValueError):
            CO.DeviceLRSchedule(bad)
    with pytest.raises(TypeError):
        CO.FusedClipAdamWWD.attach_schedule(object.__new__(CO.FusedClipAdamWWD), [0.1])
