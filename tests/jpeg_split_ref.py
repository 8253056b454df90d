"""The split decode's scheme (csrc/jpeg_split.h) restated in plain Python on a plan's own buffers, beside jpeg_ref.py: which segments
a run is cut into, what a scout walk from a guessed state meets, how the sync rounds (Jacobi steps on the exits of the round before)
converge, and what the verify pass concludes.  predict() gives the `path` value the device call must report per image -- 0 no run
split, 1 split and passed, 2 split, then decoded by the one-lane walk -- for any `rounds`.  It writes no coefficients: the output bits
have the host reader as their yardstick.  Slow and simple on purpose; not imported by the package."""
import functools

import numpy as np

MIN_SEG = 16


class _Table:
    """A rgbnm_jpeg_hufftab row, looked up as the kernel does: 9 bits first, then the canonical search over lengths 10..16."""

    def __init__(self, row):
        row = np.ascontiguousarray(row)
        self.look = row[:1024].view(np.uint16).tolist()
        self.maxcode = row[1024:1096].view(np.int32).tolist()
        self.valoff = row[1096:1168].view(np.int32).tolist()
        self.vals = row[1168:1424].tolist()


class _Run:
    def __init__(self, data, nmcu, comps, dc, ac):
        pad = bytes(-len(data) % 4 + 16)                   # reads behind the run's words give zeros
        self.big, self.nbits = int.from_bytes(data + pad, "big"), 8 * (len(data) + len(pad))
        self.total_bits, self.nmcu, self.comps, self.dc, self.ac = 8 * len(data), nmcu, comps, dc, ac

    def peek(self, pos, n):
        if n == 0:
            return 0
        if pos + n > self.nbits:                           # far behind the run: zeros
            return (self.peek(pos, self.nbits - pos) << (pos + n - self.nbits)) if pos < self.nbits else 0
        return (self.big >> (self.nbits - pos - n)) & ((1 << n) - 1)

    def symbol(self, pos, table):
        """(bits consumed, size, run nibble, value) or None for a pattern no code matches."""
        e = table.look[self.peek(pos, 9)]
        length, sym = e >> 8, e & 255
        if length == 0:
            idx = -1
            for l in range(10, 17):
                code = self.peek(pos, l)
                if code <= table.maxcode[l]:
                    length, idx = l, code + table.valoff[l]
                    break
            if idx < 0 or idx > 255:
                return None
            sym = table.vals[idx]
        s, rr = sym & 15, sym >> 4
        bits = self.peek(pos + length, s)
        val = bits - (1 << s) + 1 if s and bits < (1 << (s - 1)) else bits
        return length + s, s, rr, val


def scout_walk(run, state, end, maxtrips):
    """From state (pos, k, blk) to at or past `end`, carrying on over impossible symbols.  Returns (exit state, record) with record =
    (blocks started, blocks completed, position behind the last completed block, error anywhere, error up to that block)."""
    pos, k, blk = state
    nstart = ndone = 0
    done_pos, err, err_done = pos, False, False
    trips = 0
    while trips < maxtrips and pos < end:
        trips += 1
        comp, isdc = run.comps[blk], k == 0
        y = run.symbol(pos, run.dc[comp] if isdc else run.ac[comp])
        if y is None:                                      # unassigned code: one bit skipped, the state stays
            pos, err = pos + 1, True
            continue
        used, s, rr, _ = y
        pos += used
        if isdc and rr:                                    # a DC symbol with a run nibble: the nibble is ignored
            err, rr = True, 0
        nstart += isdc
        wr = isdc or s != 0
        kk = 0 if isdc else k + rr
        if wr and kk > 63:                                 # index past 63: clamped
            err, kk = True, 63
        k = kk + 1 if wr else (k + 16 if rr == 15 else 64)
        if k >= 64:
            k, blk = 0, (blk + 1) % len(run.comps)
            ndone, done_pos, err_done = ndone + 1, pos, err
    if pos > run.total_bits:
        err = True
    return (pos, k, blk), (nstart, ndone, done_pos, err, err_done)


def run_passes(run, seg_bits, rounds):
    """(passed, segments, segment walks) of one split run after scout, `rounds` sync rounds and verify."""
    nseg = -(-run.total_bits // seg_bits)
    ends = [min((j + 1) * seg_bits, run.total_bits) for j in range(nseg)]
    entry = [(j * seg_bits, 0, 0) for j in range(nseg)]
    walked = [scout_walk(run, entry[j], ends[j], seg_bits + 1) for j in range(nseg)]
    exits, rec, walks = [w[0] for w in walked], [w[1] for w in walked], nseg
    for _ in range(rounds):
        new = list(exits)
        for j in range(1, nseg):
            if entry[j] != exits[j - 1]:                   # the exits of the round BEFORE, whatever the order of the lanes
                entry[j] = exits[j - 1]
                new[j], rec[j] = scout_walk(run, entry[j], ends[j], seg_bits + 1)
                walks += 1
        exits = new
    converged = all(entry[j] == exits[j - 1] for j in range(1, nseg))
    total, done, found = run.nmcu * len(run.comps), 0, False
    for nstart, ndone, done_pos, err, err_done in rec:
        if done >= total:
            break                                          # behind the last block: padding bits only
        if done + ndone < total:
            if err:
                return False, nseg, walks
        else:
            if done + ndone > total or err_done or done_pos > run.total_bits or run.total_bits - done_pos > 8:
                return False, nseg, walks
            found = True
        done += ndone
    return converged and found, nseg, walks


def runs_of(plan, i):
    """The _Run objects of image i of a dct_manip.JpegBatchPlan."""
    im = plan.images[i].numpy()
    ncomp, nblk = int(im[0]), int(im[3])
    dc_tab, ac_tab = im[5:8].tolist(), im[8:11].tolist()
    comps = [int(im[17 + b]) for b in range(nblk)]
    table = functools.lru_cache(maxsize=None)(lambda t: _Table(plan.tables[t].numpy()))
    dc, ac = [table(dc_tab[c]) for c in range(ncomp)], [table(ac_tab[c]) for c in range(ncomp)]
    stream, out = plan.stream.numpy(), []
    for r in plan.runs[:plan.nruns].numpy():
        if int(r[2]) == i and int(r[4]) > 0:
            off, nbytes = int(r[0]) & 0xFFFFFFFF, int(r[1]) & 0xFFFFFFFF
            out.append(_Run(bytes(stream[off:off + nbytes]), int(r[4]), comps, dc, ac))
    return out


def predict(plan, seg_bits, rounds, min_seg=MIN_SEG):
    """(path per image, segments of the longest split run, segment walks per segment over the batch)."""
    paths, longest, walks, segs = [], 0, 0, 0
    for i in range(plan.n):
        path = 0
        if int(plan.status[i]) == 0:
            for run in runs_of(plan, i):
                if -(-run.total_bits // seg_bits) < max(2, min_seg):
                    continue
                ok, nseg, w = run_passes(run, seg_bits, rounds)
                longest, walks, segs = max(longest, nseg), walks + w, segs + nseg
                path = max(path, 1 if ok else 2)
        paths.append(path)
    return paths, longest, (walks / segs if segs else 0.0)
