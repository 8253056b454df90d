"""Element-wise kernel checking: guarded outputs, NaN-filled input gaps, a forward-error bound per element and the names of
the device kernels a call dispatched.  A plain module, imported by name from the tests (not a conftest.py).

- guarded(rows, cols, dtype, ld) allocates ONE buffer with GUARD_BYTES of margin before and after a [rows, ld] matrix and
  returns a Guarded whose .t is the strided [rows, cols] view.  Margins, the ld - cols gap and the output itself start as a
  canary: a quiet NaN with a payload.  check_guards() compares raw bits (integer views) and reports (a) any margin or gap
  element that changed and (b) any output element that still holds the canary, i.e. was never written.
- nan_padded(x, ld, extra_rows) copies an input into a buffer whose ld - cols gap and extra rows hold NaN: a kernel that lets
  them reach a result turns that result into NaN.
- check_bound(got, ref, mag, dtype, a, c_u, where) checks every element:  |got - ref| <= a ulp_T(ref) + c_u mag [+ extra].
  ref is the fp64 result of the T-rounded inputs, mag the same computation in fp64 on absolute values (the standard
  forward-error magnitude), ulp_T(x) = 2^(max(floor(log2|x|), emin_T) - p_T).  It returns the worst ratio
  |got - ref| / bound, so that a test can print the headroom it has.
- launched(fn) runs fn under torch.profiler and returns the names of the device kernels it dispatched.
"""
import math

import torch

U = 2.0 ** -24                      # unit roundoff of the fp32 accumulators
GUARD_BYTES = 64 * 1024
CANARY = {2: 0x7FC5, 4: 0x7FC0A5A5}  # quiet NaN with a payload, per element size
_INT = {2: torch.int16, 4: torch.int32}
# (precision p, emin) per element type
_FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}
# unit roundoff of the type P is rounded to before a second product (attention: P . V)
U_OF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}


def _esz(dtype):
    return torch.tensor([], dtype=dtype).element_size()


class Guarded:
    """One output matrix inside a canary-filled buffer.  .t: the [rows, cols] view (row pitch ld); .raw: integer view of the
    whole buffer; .off: element offset of the matrix in it."""

    def __init__(self, rows, cols, dtype, ld, device):
        esz = _esz(dtype)
        self.rows, self.cols, self.ld, self.dtype, self.esz = rows, cols, ld, dtype, esz
        self.off = GUARD_BYTES // esz
        n = self.off + rows * ld + self.off
        self.raw = torch.empty(n, dtype=_INT[esz], device=device)
        self.raw.fill_(CANARY[esz])
        self.canary = CANARY[esz]
        flat = self.raw.view(dtype)[self.off:self.off + rows * ld]
        self.t = flat.view(rows, ld)[:, :cols] if cols is not None else flat

    def fill_(self, values):
        """The output starts with these values instead of the canary (accumulating outputs)."""
        self.t.copy_(values)
        return self

    def check(self, where="", written=True):
        return check_guards(self, where, written)


def guarded(rows, cols, dtype, ld=None, device="cuda"):
    """cols None: a 1-D vector of `rows` elements."""
    if cols is None:
        return Guarded(rows, None, dtype, 1, device)
    ld = cols if ld is None else ld
    assert ld >= cols
    return Guarded(rows, cols, dtype, ld, device)


def check_guards(g, where="", written=True):
    """Raise AssertionError if a margin / gap element changed or (written=True) an output element still holds the canary."""
    raw, off = g.raw, g.off
    n = g.rows * g.ld
    msgs = []
    for name, part, base in (("front margin", raw[:off], -off), ("back margin", raw[off + n:], n)):
        bad = (part != g.canary).nonzero().flatten()
        if bad.numel():
            first = [int(i) + base for i in bad[:4]]
            msgs.append(f"{name}: {bad.numel()} elements changed, first at element offsets {first} from the matrix start")
    if g.cols is not None:
        body = raw[off:off + n].view(g.rows, g.ld)
        if g.ld > g.cols:
            gap = body[:, g.cols:]
            bad = (gap != g.canary).nonzero()
            if bad.numel():
                msgs.append(f"ld gap: {bad.shape[0]} elements changed, first (row, col) "
                            f"{[(int(r), g.cols + int(c)) for r, c in bad[:4]]}")
        out = body[:, :g.cols]
    else:
        out = raw[off:off + n]
    if written:
        bad = (out == g.canary).nonzero()
        if bad.numel():
            msgs.append(f"{bad.shape[0]} output elements never written, first {[tuple(int(v) for v in b) for b in bad[:4]]}")
    assert not msgs, f"{where}: " + "; ".join(msgs)


def nan_padded(x, ld=None, extra_rows=0):
    """x [rows, cols] copied into a buffer [rows + extra_rows, ld] whose gap columns and extra rows are NaN; returns the
    [rows, cols] view (row pitch ld).  The rows past `rows` stay reachable through the storage, like a larger activation."""
    rows, cols = x.shape
    ld = cols if ld is None else ld
    buf = torch.full((rows + extra_rows, ld), float("nan"), dtype=x.dtype, device=x.device)
    buf[:rows, :cols] = x
    return buf[:rows, :cols]


def ulp(x, dtype):
    """ulp_T(x) = 2^(max(floor(log2|x|), emin_T) - p_T), elementwise in fp64 (x = 0: the smallest normal's ulp)."""
    p, emin = _FMT[dtype]
    ax = x.double().abs()
    _, e = torch.frexp(ax)                         # |x| = m 2^e, m in [0.5, 1): floor(log2|x|) = e - 1
    e = torch.where(ax == 0, emin, torch.clamp(e.to(torch.int32) - 1, min=emin))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), (e - p).to(torch.int32))


def check_bound(got, ref, mag, dtype, a, c_u, where, extra=None, tile=None, verbose=True):
    """Every element:  |got - ref| <= a ulp_T(ref) + c_u mag (+ extra).  got: the kernel's output (any float dtype); ref,
    mag, extra: fp64 tensors of got's shape.  tile: (rows, cols) of the path's output tile, to name the tile of a
    violation.  Returns the worst ratio |got - ref| / bound."""
    got = got.double()
    ref = ref.double()
    bound = a * ulp(ref, dtype)
    if c_u:
        bound = bound + c_u * mag.double()
    if extra is not None:
        bound = bound + extra
    err = (got - ref).abs()
    ratio = err / bound
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = ~(err <= bound)                         # NaN in got is a violation
    nbad = int(bad.sum())
    if nbad:
        idx = bad.nonzero()
        coords = []
        for c in idx[:6]:
            c = tuple(int(v) for v in c)
            s = f"{c}: got {float(got[c]):.6g} ref {float(ref[c]):.6g} bound {float(bound[c]):.3g}"
            if tile is not None and len(c) >= 2:
                s += f" tile ({c[-2] // tile[0]}, {c[-1] // tile[1]})"
            elif tile is not None:
                s += f" tile {c[0] // tile[0]}"
            coords.append(s)
        raise AssertionError(f"{where}: {nbad} of {err.numel()} elements out of bound, worst ratio {worst:.3g}; "
                             + "; ".join(coords))
    return worst


class Worst:
    """Collects the worst ratio per key, printed at the end of a test (pytest -s, or -rA) as the bars' measured headroom."""

    def __init__(self):
        self.d = {}

    def __call__(self, key, r):
        self.d[key] = max(self.d.get(key, 0.0), r)
        return r

    def report(self, title):
        print(f"\n[{title}] worst bound ratios: " + ", ".join(f"{k}={v:.3g}" for k, v in sorted(self.d.items())))


def launched(fn):
    """(result of fn(), names of the device kernels fn dispatched)."""
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return res, names


def ran(names, *subs):
    """True if some kernel name contains every one of subs."""
    return any(all(s in n for s in subs) for n in names)
