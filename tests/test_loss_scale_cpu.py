"""CPU checks of the device loss scaler: the scale update of tests/loss_scale_ref.py against torch._amp_update_scale_ bit for
bit (and its seeded fp32-product defect caught by the same check), the clamp, the state_dict exchange with
torch.amp.GradScaler, and the C ABI of rgbnm_clip_adamw_wd_step_scaled: exported, header and binding agree, every host-side
refusal returns before anything touches the device (so they run here, on pointers that are never followed)."""
import ctypes
import os
import re

import pytest
import torch

import loss_scale_ref as LS
from rgb_no_more_amd import custom_optims as CO
from rgb_no_more_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -3
SEQ = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0]


def torch_sequence(scale, found, growth, backoff, interval):
    out, tracker = [], 0
    for f in found:
        scale, tracker = LS.torch_update_scale(scale, tracker, bool(f), growth, backoff, interval)
        out.append((scale, tracker))
    return out


def test_scale_update_matches_torch_bit_for_bit():
    want = torch_sequence(65536.0, SEQ, 1.6, 0.625, 2)
    got = LS.run_sequence(65536.0, SEQ, 1.6, 0.625, 2)
    assert got == want
    assert got[1][0] == 104857.6015625 and got[-1][0] == 167772.15625
    # the reference's constants over a longer random sequence, and a scale whose growth overflows fp32 (kept, tracker reset)
    g = torch.Generator().manual_seed(5)
    found = (torch.rand(400, generator=g) < 0.2).int().tolist()
    for interval in (1, 3, 600):
        assert LS.run_sequence(65536.0, found, 1.6, 0.625, interval) == torch_sequence(65536.0, found, 1.6, 0.625, interval)
    big = 3.0e38
    assert LS.run_sequence(big, [0, 0, 1], 1.6, 0.625, 1) == torch_sequence(big, [0, 0, 1], 1.6, 0.625, 1)
    assert LS.run_sequence(big, [0], 1.6, 0.625, 1)[0] == (float(torch.tensor(big, dtype=torch.float32)), 0)


def test_an_fp32_product_fails_the_same_check():
    """The defect the check has to catch: scale * factor taken in fp32."""
    want = torch_sequence(65536.0, SEQ, 1.6, 0.625, 2)
    bad = LS.run_sequence(65536.0, SEQ, 1.6, 0.625, 2, product="fp32")
    assert bad != want
    assert bad[-1][0] != 167772.15625


def test_clamp():
    assert LS.update_scale(2.0 ** 18, 0, False, 1.6, 0.625, 1, 2.0 ** -4, 2.0 ** 18) == (2.0 ** 18, 0)
    assert LS.update_scale(2.0 ** -4, 5, True, 1.6, 0.625, 1, 2.0 ** -4, 2.0 ** 18) == (2.0 ** -4, 0)
    assert LS.update_scale(2.0 ** 40, 0, True, 1.6, 0.625, 600, 2.0 ** -4, 2.0 ** 18) == (2.0 ** 18, 0)
    assert LS.update_scale(2.0 ** 40, 0, True, 1.6, 0.625, 600, 2.0 ** -4, float("inf")) == (2.0 ** 40 * 0.625, 0)
    # inside the range nothing moves
    assert LS.update_scale(1024.0, 0, False, 1.6, 0.625, 2, 2.0 ** -4, 2.0 ** 18) == (1024.0, 1)


def test_state_dict_round_trip_with_gradscaler():
    """torch.amp.GradScaler's keys, both directions, before any device use."""
    ref = torch.amp.GradScaler("cpu", init_scale=1024.0, growth_factor=1.6, backoff_factor=0.625, growth_interval=600)
    want = ref.state_dict()
    assert set(want) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    s = CO.DeviceLossScaler()
    assert s.get_scale() == 65536.0 and s.skipped_steps() == 0
    s.load_state_dict(want)
    assert s.state_dict() == want and s.get_scale() == 1024.0
    mine = CO.DeviceLossScaler(init_scale=4096.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=7)
    sd = mine.state_dict()
    sd["_growth_tracker"] = 3
    ref.load_state_dict(sd)
    assert ref.state_dict() == sd
    assert ref.get_growth_factor() == 2.0 and ref.get_backoff_factor() == 0.5 and ref.get_growth_interval() == 7
    back = CO.DeviceLossScaler()
    back.load_state_dict(ref.state_dict())
    assert back.state_dict() == sd
    assert CO.DeviceLossScaler(enabled=False).state_dict() == {}
    with pytest.raises(RuntimeError):
        s.load_state_dict({})


def test_defaults_are_the_reference_values_and_step_wants_the_fused_optimizer():
    s = CO.DeviceLossScaler()
    assert (s._growth_factor, s._backoff_factor, s._growth_interval, s._scale_min, s._scale_max) == (1.6, 0.625, 600, 2.0 ** -4, 2.0 ** 18)
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(TypeError):
        s.step(torch.optim.AdamW([p]))
    with pytest.raises(TypeError):
        CO.DeviceLossScaler(enabled=False).step(torch.optim.SGD([p], lr=0.1))
    loss = torch.tensor(3.0)
    assert CO.DeviceLossScaler(enabled=False).scale(loss) is loss
    assert CO.DeviceLossScaler(enabled=False).update() is None and s.update() is None
    assert "inside step" in CO.DeviceLossScaler.update.__doc__


# ------------------------------------------------------------------------------------------------------------------- ABI
CTYPE = {"float*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "const unsigned char*": ctypes.c_void_p,
         "rgbnm_loss_scale_state*": ctypes.c_void_p, "void*": ctypes.c_void_p, "long long": ctypes.c_longlong,
         "float": ctypes.c_float, "double": ctypes.c_double, "int": ctypes.c_int, "size_t": ctypes.c_size_t}


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
        typ = re.sub(r"\s*\b\w+$", "", a)               # drop the parameter's name
        args.append(typ.replace(" *", "*"))
    return m.group(1).strip(), args


def test_symbols_header_and_binding_agree():
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in ("rgbnm_clip_adamw_wd_step_scaled", "rgbnm_clip_adamw_wd_scaled_workspace"):
        assert hasattr(dll, name), name
        ret, args = header_args(name)
        res, argtypes = L.PROTOTYPES[name]
        assert res is CTYPE[ret], (name, ret)
        assert [CTYPE[a] for a in args] == argtypes, (name, args)
    # the unscaled entry's arguments minus `step`, then state, factors (double), interval, clamp, workspace, stream
    _, old = header_args("rgbnm_clip_adamw_wd_step")
    _, new = header_args("rgbnm_clip_adamw_wd_step_scaled")
    assert len(old) == 17 and old[10] == "int"
    assert new == old[:10] + old[11:14] + ["rgbnm_loss_scale_state*", "double", "double", "int", "float", "float"] + old[14:]
    assert L.lib().rgbnm_abi_version() == 3
    ws = L.lib().rgbnm_clip_adamw_wd_scaled_workspace()
    assert ws >= 256 * 4 + 8 and ws % 4 == 0            # the 256 partial sums, then at least inv and step
    # the state block: five named words at the documented offsets, 32 bytes
    m = re.search(r"typedef struct rgbnm_loss_scale_state \{(.*?)\} rgbnm_loss_scale_state;", header(), flags=re.S)
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields[:5] == ["float scale", "int growth_tracker", "int step", "int skipped", "float found_inf"]
    assert fields[5:] == ["int reserved[3]"]


def test_refusals_return_before_any_device_call():
    lib = L.lib()
    wsb = lib.rgbnm_clip_adamw_wd_scaled_workspace()
    ok = dict(p=0x1000, g=0x2000, m=0x3000, v=0x4000, fl=0x5000, n=512, norm=None, state=0x6000, growth=1.6, backoff=0.625,
              interval=600, smin=2.0 ** -4, smax=2.0 ** 18, ws=0x7000, wsb=wsb)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.rgbnm_clip_adamw_wd_step_scaled(a["p"], a["g"], a["m"], a["v"], a["fl"], a["n"], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0,
                                                   a["norm"], a["state"], a["growth"], a["backoff"], a["interval"], a["smin"],
                                                   a["smax"], a["ws"], a["wsb"], None)
    for k in ("p", "g", "m", "v", "fl", "state", "ws"):
        assert call(**{k: None}) == EINVAL, k
    for n in (500, 0, -256, 257):
        assert call(n=n) == EINVAL, n
    for wsb_ in (0, 1024, wsb - 4):
        assert call(wsb=wsb_) == EWORKSPACE, wsb_
    for interval in (0, -1):
        assert call(interval=interval) == EINVAL, interval
    for f in (0.0, -1.6, float("nan")):
        assert call(growth=f) == EINVAL, f
        assert call(backoff=f) == EINVAL, f
    assert call(smin=2.0, smax=1.0) == EINVAL
    assert call(smin=float("nan")) == EINVAL and call(smax=float("nan")) == EINVAL
    # several faults at once are still a refusal; a short workspace with bad arguments is EINVAL (arguments are checked first)
    assert call(p=None, wsb=0) == EINVAL
