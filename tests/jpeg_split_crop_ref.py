"""What the split decode for crop boxes (rgbnm_jpeg_decode_batch_split_crop) must report, restated in numpy beside jpeg_split_ref.py
and jpeg_crop_ref.py: the passes of jpeg_split_ref with the segment records kept -- the first block that starts in every segment --
the live test by looking at every MCU of a segment (the kernel's is closed form), and from both the `path`, `seg_live` and `walked`
arrays of a call.  Also the damaged streams the tests feed: a well-formed file with bytes of its scan overwritten.  Slow and simple on
purpose; a plain module, imported by name."""
import functools

import numpy as np

import jpeg_cases as JC
import jpeg_crop_ref as CR
import jpeg_ref as JR
import jpeg_split_ref as SR
import jpeg_writer as JW

SETTINGS = [(256, 0), (1024, 2)]                  # (seg_bits, option "jpeg_min_seg"; 0: the default, 16): the split tests' two


def need(m, mcus_x, sampling, box):
    """bool per MCU index of m: the MCU holds a block inside its component's box (jpeg_crop_ref.expected_walked's predicate)."""
    m = np.asarray(m)
    mx, my = m % mcus_x, m // mcus_x
    out = np.zeros(m.shape, dtype=bool)
    for c, (hs, vs) in enumerate(sampling):
        t, l, h, w = [int(v) // 2 for v in box] if c else [int(v) for v in box]
        out |= (mx * hs < l + w) & (mx * hs + hs > l) & (my * vs < t + h) & (my * vs + vs > t)
    return out


def seg_is_live(b0, nstart, mcu0, nmcu, nblk, mcus_x, sampling, box):
    """Segment with blocks [b0, b0 + nstart) of a run over MCUs [mcu0, mcu0 + nmcu): does one of them, cut to the run's nmcu * nblk
    blocks, belong to a needed MCU?"""
    end = min(b0 + nstart, nmcu * nblk)
    if b0 >= end:
        return False
    return bool(need(mcu0 + np.arange(b0, end) // nblk, mcus_x, sampling, box).any())


def run_records(run, seg_bits, rounds):
    """jpeg_split_ref.run_passes with the records kept: (passed, [(b0, nstart) per segment])."""
    nseg = -(-run.total_bits // seg_bits)
    ends = [min((j + 1) * seg_bits, run.total_bits) for j in range(nseg)]
    entry = [(j * seg_bits, 0, 0) for j in range(nseg)]
    walked = [SR.scout_walk(run, entry[j], ends[j], seg_bits + 1) for j in range(nseg)]
    exits, rec = [w[0] for w in walked], [w[1] for w in walked]
    for _ in range(rounds):
        new = list(exits)
        for j in range(1, nseg):
            if entry[j] != exits[j - 1]:
                entry[j] = exits[j - 1]
                new[j], rec[j] = SR.scout_walk(run, entry[j], ends[j], seg_bits + 1)
        exits = new
    passed = all(entry[j] == exits[j - 1] for j in range(1, nseg))
    total, done, found, b0, segs = run.nmcu * len(run.comps), 0, False, 0, []
    for nstart, _, _, _, _ in rec:
        segs.append((b0, nstart))
        b0 += nstart
    for nstart, ndone, done_pos, err, err_done in rec:
        if done >= total:
            break
        if done + ndone < total:
            if err:
                passed = False
                break
        else:
            if done + ndone > total or err_done or done_pos > run.total_bits or run.total_bits - done_pos > 8:
                passed = False
                break
            found = True
        done += ndone
    return passed and found, segs


def records(plan, seg_bits, rounds, min_seg=SR.MIN_SEG, check=True):
    """What does not depend on the boxes: (path per image, {run index: segments [(b0, nstart)]} for the split runs).  One trip over
    the run records; only runs long enough to be split are looked at.  check: the path equals jpeg_split_ref.predict's (which
    takes a trip over all records per image: not for thousands of runs)."""
    paths, segs, tables, per_image = [0] * plan.n, {}, {}, {}
    stream = plan.stream.numpy()

    def table(t):
        if t not in tables:
            tables[t] = SR._Table(plan.tables[t].numpy())
        return tables[t]

    for ri, r in enumerate(plan.runs[:plan.nruns].numpy()):
        i, nmcu = int(r[2]), int(r[4])
        off, nbytes = int(r[0]) & 0xFFFFFFFF, int(r[1]) & 0xFFFFFFFF
        if nmcu <= 0 or int(plan.status[i]) != 0 or -(-8 * nbytes // seg_bits) < max(2, min_seg):
            continue
        if i not in per_image:                                 # as jpeg_split_ref.runs_of reads the image record
            im = plan.images[i].numpy()
            ncomp, nblk = int(im[0]), int(im[3])
            per_image[i] = ([int(im[17 + b]) for b in range(nblk)], [table(int(im[5 + c])) for c in range(ncomp)],
                            [table(int(im[8 + c])) for c in range(ncomp)])
        comps, dc, ac = per_image[i]
        ok, segs[ri] = run_records(SR._Run(bytes(stream[off:off + nbytes]), nmcu, comps, dc, ac), seg_bits, rounds)
        paths[i] = max(paths[i], 1 if ok else 2)
    if check:
        assert paths == SR.predict(plan, seg_bits, rounds, min_seg)[0]
    return paths, segs


def longest(plan, seg_bits, min_seg=SR.MIN_SEG):
    """Segments of the longest run that is split (0: none): rounds >= longest - 1 makes convergence certain."""
    n = [-(-8 * (int(r[1]) & 0xFFFFFFFF) // seg_bits) for r in plan.runs[:plan.nruns].numpy() if int(r[4]) > 0 and int(plan.status[int(r[2])]) == 0]
    return max([v for v in n if v >= max(2, min_seg)], default=0)


def expected(plan, recs, boxes):
    """(seg_live, walked) int32 [nruns] for one box per image, from records(): a split run of a path 1 image counts its live segments
    and is not walked by one lane; in such an image a run that was not split is walked to its end; every other run is walked as the
    plain crop call walks it (jpeg_crop_ref.expected_walked)."""
    paths, segs = recs
    runs, images = plan.runs[:plan.nruns].numpy(), plan.images[:plan.n].numpy()
    live, walked = np.zeros(plan.nruns, dtype=np.int32), np.zeros(plan.nruns, dtype=np.int32)
    for ri, r in enumerate(runs):
        i, mcu0, nmcu = int(r[2]), int(r[3]), int(r[4])
        if nmcu == 0 or int(plan.status[i]) != 0:
            continue
        im = images[i]
        ncomp, mcus_x, nblk = int(im[0]), int(im[1]), int(im[3])
        sampling = [(int(im[11 + c]), int(im[14 + c])) for c in range(ncomp)]
        if paths[i] == 1 and ri in segs:
            live[ri] = sum(seg_is_live(b0, ns, mcu0, nmcu, nblk, mcus_x, sampling, boxes[i]) for b0, ns in segs[ri])
        elif paths[i] == 1:
            walked[ri] = nmcu
        else:
            walked[ri] = CR.expected_walked(mcu0, nmcu, mcus_x, sampling, boxes[i])
    return live, walked


def total_segments(recs, plan):
    """Segments of the split runs of path 1 images."""
    paths, segs = recs
    runs = plan.runs[:plan.nruns].numpy()
    return sum(len(s) for ri, s in segs.items() if paths[int(runs[ri][2])] == 1)


# ---- damaged streams: a file the parser still accepts whose scan no longer decodes ------------------------------------------------
def scan_span(data):
    """(first, last + 1) byte of the entropy-coded data of a single-scan file."""
    p = 2
    while data[p + 1] != 0xDA:
        assert data[p] == 0xFF
        p += 2 + ((data[p + 2] << 8) | data[p + 3])
    first = p + 2 + ((data[p + 2] << 8) | data[p + 3])
    return first, data.rindex(b"\xff\xd9")


def damage(data, share, value=0x5A, count=3):
    """`count` bytes of the scan from `share` (0..1) of its length overwritten with `value`: never FF, and not behind an FF, so the
    byte scan sees the markers it saw (the run lengths may change where a stuffed FF 00 loses its FF: bytes at FF are left alone)."""
    first, end = scan_span(data)
    out = bytearray(data)
    at = first + int(share * (end - first))
    done = 0
    while done < count and at < end - 1:
        if out[at] != 0xFF and out[at - 1] != 0xFF:
            out[at] = value
            done += 1
        at += 1
    assert done == count
    return bytes(out)


# ---- the file sets of the kernel tests: name -> (files, grid); every set holds a file long enough to be split in both SETTINGS --------
def repack(data):
    """The file's kept coefficients written again as ONE run (no restart interval) behind the same tables; the MCU padding is zero."""
    f = JR.parse(data)
    Y, C, quant = JR.decode_file(data)
    nc = f["ncomp"]
    sampling = list(zip(f["hs"], f["vs"])) if nc == 3 else [(1, 1)]
    planes = []
    for kept, (gh, gw) in zip([Y] + ([C[0], C[1]] if nc == 3 else []), JW.padded_grids(f["width"], f["height"], sampling)):
        p = np.zeros((gh, gw, 64), np.int64)
        p[:kept.shape[0], :kept.shape[1]] = kept
        planes.append(p)
    tables = [(JW.bits_vals(f["dc"][c]), JW.bits_vals(f["ac"][c])) for c in range(nc)]
    q = [[int(v) for v in quant[c]] for c in range(nc)]
    return JW.write(planes, q, sampling, tables, f["width"], f["height"], dqt16=any(v > 255 for t in q for v in t))


@functools.lru_cache(maxsize=None)
def file_sets():
    """pillow: jpeg_cases.pillow_files() on (9, 13).  small: grid (5, 7) -- the layouts that have this grid (component ids, the gray
    sampling bytes), the stuffing family (FF bytes in the data; one 4:2:0, two one-component files), each as written (restart markers:
    short runs) and again as one run, and a marker-less colour and gray Pillow file.  padding: grid (5, 11), content in the MCU
    padding on both edges.  tables: grid (8, 12), long_codes behind six tables of its own beside standard-table files of 1, 4 and 24
    runs.  many: jpeg_cases.many_runs() (8275 short runs, none split) with two marker-less files in the middle of the batch."""
    lay, stuff = JC.layouts(), JC.stuffing()
    small = [lay["420_ids"].data, lay["gray_0x22"].data, lay["gray_0x11"].data] + [s.data for s in stuff]
    small += [repack(d) for d in small] + [JC.encode(JC.noisy(37, 53, 5), quality=95), JC.encode(JC.noisy(37, 53, 6, gray=True), quality=95)]
    many = [s.data for s in JC.many_runs()]
    many[100:100] = [JC.encode(JC.noisy(37, 53, 7), quality=95), JC.encode(JC.noisy(37, 53, 8, gray=True), quality=96)]
    return {"pillow": (list(JC.pillow_files().values()), (9, 13)), "small": (small, (5, 7)),
            "padding": ([lay["420_padding"].data, JC.encode(JC.noisy(35, 83, 9), quality=90)], (5, 11)),
            "tables": ([JC.long_codes().data] + [JC.standard_420(40 + k, w=96, h=64, restart=r).data for k, r in enumerate((1, 6, 0))], (8, 12)),
            "many": (many, (5, 7))}


def rounds_for(plan, seg_bits, min_seg):
    """The tests' choice: as many rounds as certain convergence needs, at most the 64 the call takes."""
    return min(64, max(0, longest(plan, seg_bits, min_seg) - 1))


@functools.lru_cache(maxsize=None)
def damaged_set():
    """Grid (8, 8): well-formed marker-less files, each also with bytes overwritten early, in the middle and near the end of its scan
    (the one-lane walk of most of them ends in an error), a gray one, and a file with a marker per MCU row damaged in its second run."""
    a, b, g = JC.encode(JC.noisy(64, 64, 31), quality=92), JC.encode(JC.noisy(64, 64, 32), quality=96), JC.encode(JC.noisy(64, 64, 33, gray=True), quality=95)
    rows = JC.encode(JC.noisy(64, 64, 34), quality=95, restart_marker_rows=1)
    return [a, damage(a, 0.1), damage(a, 0.5), damage(a, 0.93), b, damage(b, 0.6, value=0x00), g, damage(g, 0.7), damage(rows, 0.4), rows], (8, 8)
