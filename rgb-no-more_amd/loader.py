"""Batched host reader + H2D staging for the DCT datasets.

Replaces, for `--domain DCT`, the reference's per-sample path
    imagenet_dataset_indexing.__getitem__ (datasets.py:274-297: read_coefficients + dequantise per sample, CPU tensors)
    -> DistributedSampler / DataLoader workers / default collate (datasets.py:533-546)
    -> pipeline_utils.unpack_data (.to(device), pipeline_utils.py:70-73)
with one object:

    loader = DCTBatchLoader(paths, labels, batch_size=256, device="cuda:0", rank=rank, world_size=world,
                            transform=rg.datasets.get_transform("imagenet_dct", "train", fused=True, ...))
    for epoch in range(E):
        loader.set_epoch(epoch)                       # = trainloader.sampler.set_epoch(epoch), train.py:143
        for (Y, CbCr), labels in loader:              # device tensors, ToRange'd -- what unpack_data returns
            ...

How: a decoder thread calls `librgbnm_reader.so`'s pthread batch entry (entropy decode only, GIL released) straight into a
RING of re-used pinned int16 batch buffers, `prefetch` batches ahead of the consumer; the consumer issues ONE H2D copy per
tensor on a side stream, waits for it with an event (so the pinned buffer can go back to the ring), and runs the fused HIP
transform (de-quantise + crop + resize + flip + RandAugment + ToRange) on the raw coefficients.  No per-sample tensors, no
collate, no worker processes.  Sharding follows torch's DistributedSampler(shuffle, drop_last=False) index for index
(seed + epoch permutation, padded by wrapping, rank-strided), so a run is reproducible against the reference's sampler.

`crop_on_host=True` (train transform only): the crop boxes and the augmentation draws of a batch are sampled BEFORE its files
are decoded, the reader copies only each file's crop box out of libjpeg's coefficient arrays, back to back into flat pinned
buffers, and ONE H2D copy of the used prefix ships the batch: 787 KB -> ~380 KB per image on the sampler's mix of crop sides
("768 KB/img raw coefficients also make PCIe the next limit -- crop on host before H2D, or ship only the crop
box").  The kernels read the packed boxes in place (rgbnm_dct_augment_packed): same output bits as the whole-grid path.

`decode="device"` (default "host"): the producer thread reads the files and only FINDS their independent bit streams
(dct_manip.prepare_jpeg_batch: a byte scan into a pinned ring of plans); the consumer ships the compressed bytes -- a tenth of the
coefficients -- and launches the Huffman walk on a side stream (csrc/jpeg_decode.hip, one lane per restart run), up to `prefetch`
batches ahead, each on a stream of its own, without a host sync; the step's stream waits on the batch's event.  The transform gets
the same whole-grid tensors, bit for bit.  A file the device path refuses (progressive, ...) is decoded by the host reader and
uploaded into its slot.  The device status of a batch comes back through a pinned copy and is looked at once it has arrived, a
batch or more later; a negative one raises, naming the file.  Not combinable with crop_on_host.
`crop_on_device=True` (with decode="device" and the train transform only): crop_on_host's idea on the device's side.  The producer
draws the batch's boxes and augmentation parameters before it prepares the plan, the boxes travel with it, and the launch is the crop
decode (dct_manip.launch_jpeg_decode(boxes=...)): restart runs outside a file's box are not walked, the others stop after the last MCU
the box needs, and only the boxes are stored, packed as the host crop reader packs them; the transform reads them in place
(apply_packed).  Same output bits as crop_on_host=True at the same seed and epoch.  A file's status then says nothing about stream
bytes behind the last MCU its box needed.  Files without restart markers are walked by one lane each up to that MCU (jpeg_split takes
no box: not combinable); the gain comes from restart markers.
`crop_on_device="split"` (same conditions, jpeg_split stays False): the crop launch is the split decode for crop boxes
(dm.launch_jpeg_split_crop) -- for files WITHOUT restart markers: their runs are cut into bit segments, and only the segments that hold
a block of a file's box are walked for the stores.  Same output bits; `.crop_on_device` is True and `.crop_split` says which launch.
`jpeg_split=True` (with decode="device" only): the launch is the split decode (dct_manip.launch_jpeg_decode(split=True)): runs of
files without restart markers are cut into bit segments, one lane each; the same tensors, bit for bit.

Everything except the H2D copy and the transform is host logic and runs (and is tested) without a GPU: with device="cpu"
the loader yields the raw (Yq, CbCrq, quant) batches.  Files must share one coefficient grid (default 64 x 64 luma blocks =
512 x 512, the pre-resized layout of the reference's dataset, README "resize to 512"); a file with another grid or an
unreadable file raises at the batch that contains it, naming the file (the reference raises inside a worker)."""
import math
import queue
import threading

import torch

from . import dct_manip as dm


class DCTBatchLoader:
    def __init__(self, paths, labels, batch_size, device="cuda", grid=(64, 64), threads=None, prefetch=2, shuffle=True,
                 seed=0, rank=0, world_size=1, drop_last=False, transform=None, crop_on_host=False, decode="host", jpeg_split=False,
                 crop_on_device=False):
        if len(paths) != len(labels):
            raise ValueError("paths and labels differ in length")
        if batch_size <= 0 or prefetch < 1:
            raise ValueError("batch_size and prefetch must be positive")
        self.paths, self.labels = list(paths), torch.as_tensor(labels, dtype=torch.int64)
        self.batch_size, self.grid, self.prefetch = batch_size, tuple(grid), int(prefetch)
        self.threads = int(threads) if threads else dm.default_threads()
        self.shuffle, self.seed, self.rank, self.world_size, self.drop_last = shuffle, seed, rank, world_size, drop_last
        self.device = torch.device(device)
        self.transform = transform
        self.crop_on_host = bool(crop_on_host)
        if self.crop_on_host:
            from . import custom_transforms as CT
            if not isinstance(transform, CT.TrainTransform_DCT) or transform.eval_mode or self.device.type != "cuda":
                raise ValueError("crop_on_host needs the fused train transform (TrainTransform_DCT) and a HIP device: the crop "
                                 "boxes are drawn before the decode; the eval transform reads the whole grid")
        if decode not in ("host", "device"):
            raise ValueError(f'decode must be "host" or "device", got {decode!r}')
        if crop_on_device not in (False, True, "split"):
            raise ValueError(f'crop_on_device must be False, True or "split", got {crop_on_device!r}')
        self.crop_on_device = bool(crop_on_device)
        self.crop_split = crop_on_device == "split"          # the crop launch is the split decode's (launch_jpeg_split_crop)
        if self.crop_on_device and self.crop_on_host:
            raise ValueError("crop_on_device and crop_on_host are the same crop on the two sides of PCIe: choose one")
        if decode == "device" and self.crop_on_host:
            raise ValueError('decode="device" ships the compressed bytes, a tenth of the coefficients: there is nothing left to crop '
                             "before PCIe (crop_on_host=True belongs to the host decode; crop_on_device=True lets the device decode walk "
                             "and store only the crop boxes)")
        if self.crop_on_device:
            from . import custom_transforms as CT
            if decode != "device":
                raise ValueError('crop_on_device=True is the crop of the DEVICE decode: it needs decode="device"')
            if jpeg_split:
                raise ValueError("crop_on_device=True cannot be combined with jpeg_split=True: the whole-grid split decode takes no crop "
                                 'box (its scout and sync passes must see the whole run); crop_on_device="split" with jpeg_split=False '
                                 "is the split decode for crop boxes")
            if not isinstance(transform, CT.TrainTransform_DCT) or transform.eval_mode or self.device.type != "cuda":
                raise ValueError("crop_on_device needs the fused train transform (TrainTransform_DCT) and a HIP device: the crop "
                                 "boxes are drawn before the decode; the eval transform reads the whole grid")
        if decode == "device" and self.device.type != "cuda":
            raise ValueError('decode="device" needs a HIP device')
        if jpeg_split and decode != "device":
            raise ValueError('jpeg_split=True cuts the runs of the DEVICE decode into segments: it needs decode="device"')
        self.decode, self.jpeg_split = decode, bool(jpeg_split)
        self.h2d_bytes = 0
        self.last_packed = None        # crop_on_host / crop_on_device: the (packed parameters, nops) of the batch yielded last (tests)
        self.epoch = 0
        n = len(self.paths)
        # DistributedSampler(drop_last=False): every rank gets ceil(n / world) indices, the list is padded by wrapping
        self.num_samples = math.ceil(n / world_size) if n else 0
        self.total_size = self.num_samples * world_size
        self._ring = None

    # ---- sampler semantics (torch.utils.data.distributed.DistributedSampler.__iter__)
    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self):
        n = len(self.paths)
        if n == 0:
            return []
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            idx = torch.randperm(n, generator=g).tolist()
        else:
            idx = list(range(n))
        pad = self.total_size - len(idx)
        if pad > 0:
            idx += (idx * math.ceil(pad / len(idx)))[:pad]
        return idx[self.rank:self.total_size:self.world_size]

    def __len__(self):
        if self.drop_last:
            return self.num_samples // self.batch_size
        return math.ceil(self.num_samples / self.batch_size)

    # ---- staging ring: prefetch queued + one being consumed + one being filled
    def _buffers(self):
        if self._ring is None:
            pin = self.device.type == "cuda"
            if self.decode == "device":      # queued + launched but not yet uploaded + one being filled
                self._ring = [dm.JpegBatchPlan(self.batch_size, self.grid, pin_memory=True) for _ in range(2 * self.prefetch + 1)]
                return self._ring
            alloc = dm.alloc_packed if self.crop_on_host else dm.alloc_batch
            self._ring = [alloc(self.batch_size, self.grid, pin_memory=pin) for _ in range(self.prefetch + 2)]
        return self._ring

    # ---- decode="device": the producer finds the runs, the device walks them
    def _prepare_device(self, plan, bi):
        """Producer side of one batch: file bytes -> plan (pinned ring slot).  A file the device cannot take is decoded by the host
        reader here; its tensors travel with the item and are uploaded into its slot."""
        if getattr(plan, "busy", None) is not None:
            plan.busy.synchronize()          # the H2D copies of the slot's last batch
            plan.busy = None
        names = [self.paths[i] for i in bi]
        datas, _ = dm._jpeg_bytes(names)
        dm.prepare_jpeg_batch(datas, self.grid, out=plan, threads=min(self.threads, 16))
        plan.names = names
        hb, wb = self.grid
        fallback = []
        for k in (plan.status[:plan.n] != 0).nonzero().flatten().tolist():
            try:
                _, q, y, c = dm.read_coefficients_bytes(datas[k])
            except dm.libjpeg_exception as e:
                raise dm.libjpeg_exception(f"{names[k]}: {e}") from None
            if tuple(y.shape) != (1, hb, wb, 8, 8) or (c is not None and tuple(c.shape) != (2, (hb + 1) // 2, (wb + 1) // 2, 8, 8)):
                raise dm.libjpeg_exception(f"{names[k]}: reader error -4 (coefficient grid differs from the batch shape)")
            q3 = torch.ones((3, 8, 8), dtype=torch.int16)
            q3[:q.shape[0]] = q
            fallback.append((k, y, c, q3))
        return plan, fallback

    def _prepare_crop(self, sampler, plan, fallback):
        """crop_on_device, producer side: the batch's parameters, drawn as the crop_on_host path draws them, and what the crop launch
        needs of them in ONE pinned tensor (boxes int32 [n, 4] | y_off int64 [n] | c_off int64 [n]).  A file the host reader decoded
        is cut to its box here."""
        n = plan.n
        packed, nops = sampler.sample(n, self.grid[0], self.grid[1])
        bx = torch.from_numpy(packed["crop"].astype("int32"))
        y_off, c_off, ny, ncc = dm.packed_offsets(bx)
        meta = torch.empty(4 * n, dtype=torch.int64).pin_memory()
        meta[:2 * n].view(torch.int32).copy_(bx.reshape(-1))
        meta[2 * n:3 * n] = y_off
        meta[3 * n:] = c_off
        cut = []
        for k, y, c, q in fallback:
            t, l, h, w = bx[k].tolist()
            yc = y[0, t:t + h, l:l + w].contiguous().view(-1)
            cc = None if c is None else c[:, t // 2:(t + h) // 2, l // 2:(l + w) // 2].contiguous().view(-1)
            cut.append((k, int(y_off[k]), yc, int(c_off[k]), 2 * (h // 2) * (w // 2) * 64, cc, q))
        return packed, nops, meta, ny, ncc, cut

    def _launch_device_crop(self, plan, crop, lab, stream):
        """Consumer side of crop_on_device: uploads and the crop launch on a side stream; nothing here waits for the device."""
        packed, nops, meta, ny, ncc, cut = crop
        n = plan.n
        with torch.cuda.stream(stream):
            dev = dm.upload_jpeg_plan(plan, self.device)
            mdev = meta.to(self.device, non_blocking=True)
            boxes, yo, co = mdev[:2 * n].view(torch.int32).view(n, 4), mdev[2 * n:3 * n], mdev[3 * n:]
            Yp = torch.empty(ny, dtype=torch.int16, device=self.device)
            Cp = torch.empty(ncc, dtype=torch.int16, device=self.device)
            Q, st = dev[4], dev[5]
            if self.crop_split:
                dm.launch_jpeg_split_crop(plan, dev, (Yp, Cp, Q, st), boxes, (yo, co, ny, ncc))
            else:
                dm.launch_jpeg_decode(plan, dev, (Yp, Cp, Q, st), boxes=boxes, packed_out=(yo, co, ny, ncc))
            for t in dev[:4]:
                t.record_stream(stream)
            for k, y0, yc, c0, csz, cc, q in cut:      # refused by prepare: the kernel leaves these slots alone
                Yp[y0:y0 + yc.numel()].copy_(yc, non_blocking=True)
                if cc is None:
                    Cp[c0:c0 + csz].zero_()
                else:
                    Cp[c0:c0 + csz].copy_(cc, non_blocking=True)
                Q[k].copy_(q, non_blocking=True)
                st[k] = 0
            ld = lab.to(self.device, non_blocking=True)
            st_host = torch.empty(n, dtype=torch.int32, pin_memory=True)
            st_host.copy_(st, non_blocking=True)
            done = torch.cuda.Event()
            done.record(stream)
        plan.busy = done
        self.h2d_bytes = plan.h2d_bytes() + meta.numel() * 8
        return (Yp, Cp, Q, ld, (packed, nops, yo, co)), (done, st_host, list(plan.names))

    def _launch_device(self, plan, fallback, lab, stream):
        """Consumer side: uploads and the decode launch on a side stream; nothing here waits for the device."""
        with torch.cuda.stream(stream):
            Y, C, Q, st = dm.decode_jpeg_batch(plan, self.device, split=self.jpeg_split)
            for k, y, c, q in fallback:          # refused by prepare: the kernel leaves these slots alone
                Y[k].copy_(y, non_blocking=True)
                if c is None:
                    C[k].zero_()
                else:
                    C[k].copy_(c, non_blocking=True)
                Q[k].copy_(q, non_blocking=True)
                st[k] = 0
            ld = lab.to(self.device, non_blocking=True)
            st_host = torch.empty(plan.n, dtype=torch.int32, pin_memory=True)
            st_host.copy_(st, non_blocking=True)
            done = torch.cuda.Event()
            done.record(stream)
        plan.busy = done
        self.h2d_bytes = plan.h2d_bytes()
        return (Y, C, Q, ld, None), (done, st_host, list(plan.names))

    @staticmethod
    def _check_status(pending, wait):
        """Raise for the first batch whose device status (read back through a pinned copy) holds a negative code.  wait=False: only
        batches whose copy has arrived are looked at, so the step is never stalled."""
        while pending and (wait or pending[0][0].query()):
            done, st, names = pending.pop(0)
            done.synchronize()
            bad = (st != 0).nonzero().flatten().tolist()
            if bad:
                raise dm.libjpeg_exception(f"{names[bad[0]]}: device decode error {int(st[bad[0]])} "
                                           f"({dm.jpeg_status_text(st[bad[0]])}; {len(bad)} of {len(names)} files failed)")

    def __iter__(self):
        idx = self.indices()
        nb = len(self)
        batches = [idx[b * self.batch_size:(b + 1) * self.batch_size] for b in range(nb)]
        ring = self._buffers()
        q = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()
        sampler = None
        if self.crop_on_host or self.crop_on_device:
            from . import custom_transforms as CT
            # one stream of draws per (seed, epoch, rank): the producer samples a batch's parameters before decoding it
            sampler = CT.FastParamSampler(self.transform, seed=[self.seed, self.epoch, self.rank])

        def producer():
            try:
                for k, bi in enumerate(batches):
                    if stop.is_set():
                        return
                    buf = ring[k % len(ring)]
                    if self.decode == "device":
                        plan, fallback = self._prepare_device(buf, bi)
                        crop = self._prepare_crop(sampler, plan, fallback) if self.crop_on_device else None
                        item = ((plan, fallback, crop), self.labels[bi])
                    elif sampler is not None:
                        packed, nops = sampler.sample(len(bi), self.grid[0], self.grid[1])
                        Yp, Cp, Qp, yo, co = dm.read_coefficients_batch_crop([self.paths[i] for i in bi], packed["crop"],
                                                                             threads=self.threads, grid=self.grid, out=buf)
                        item = ((Yp, Cp, Qp, yo, co, packed, nops), self.labels[bi])
                    else:
                        view = tuple(t[:len(bi)] for t in buf)          # the last batch of an epoch may be short
                        out = dm.read_coefficients_batch([self.paths[i] for i in bi], threads=self.threads, grid=self.grid, out=view)
                        item = (out, self.labels[bi])
                    while not stop.is_set():
                        try:
                            q.put(item, timeout=0.1)
                            break
                        except queue.Full:
                            pass
                q.put(None)
            except BaseException as e:       # noqa: BLE001 -- delivered to the consumer, which re-raises it
                q.put(e)

        th = threading.Thread(target=producer, daemon=True, name="rgbnm-dct-decoder")
        th.start()
        copy_stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        try:
            if self.decode == "device":
                # up to `prefetch` batches are uploaded and decoded ahead, each on a side stream of its own: a batch without restart
                # markers is 256 long walks, and several of them run beside each other and beside the step
                streams = [torch.cuda.Stream(self.device) for _ in range(self.prefetch)]
                inflight, pending, launched, ended = [], [], 0, False
                while True:
                    while not ended and len(inflight) < self.prefetch:
                        try:
                            item = q.get(block=not inflight)
                        except queue.Empty:
                            break
                        if item is None:
                            ended = True
                            break
                        if isinstance(item, BaseException):
                            raise item
                        (plan, fallback, crop), lab = item
                        st = streams[launched % len(streams)]
                        launched += 1
                        inflight.append((st,) + (self._launch_device_crop(plan, crop, lab, st) if crop is not None else
                                                 self._launch_device(plan, fallback, lab, st)))
                    if not inflight:
                        self._check_status(pending, wait=True)
                        return
                    st, (Yd, Cd, Qd, ld, crop), check = inflight.pop(0)
                    cur = torch.cuda.current_stream(self.device)
                    cur.wait_event(check[0])
                    for t in (Yd, Cd, Qd, ld) + (crop[2:] if crop is not None else ()):
                        t.record_stream(cur)
                    self._check_status(pending, wait=False)      # the batches before this one, as far as their status has arrived
                    pending.append(check)
                    if crop is not None:
                        from . import custom_transforms as CT
                        self.last_packed = crop[:2]
                        yield tuple(CT.apply_packed(self.transform, Yd, Cd, Qd, crop[0], crop[1], y_off=crop[2], c_off=crop[3],
                                                    grid=self.grid)), ld
                        continue
                    yield self._finish(Yd, Cd, Qd, ld)
            while True:
                item = q.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                if sampler is not None:
                    from . import custom_transforms as CT
                    (Yp, Cp, Qp, yo, co, packed, nops), lab = item
                    with torch.cuda.stream(copy_stream):
                        dev = [t.to(self.device, non_blocking=True) for t in (Yp, Cp, Qp, yo.pin_memory(), co.pin_memory(), lab)]
                    copy_stream.synchronize()          # the pinned buffers go back to the decoder ring after this
                    for t in dev:
                        t.record_stream(torch.cuda.current_stream(self.device))
                    self.last_packed = (packed, nops)
                    self.h2d_bytes = 2 * (Yp.numel() + Cp.numel())
                    yield tuple(CT.apply_packed(self.transform, dev[0], dev[1], dev[2], packed, nops, y_off=dev[3], c_off=dev[4],
                                                grid=self.grid)), dev[5]
                    continue
                (Y, C, Q), lab = item
                if copy_stream is None:
                    yield self._finish(Y.clone(), C.clone(), Q.clone(), lab)     # host buffers are recycled: hand out copies
                    continue
                with torch.cuda.stream(copy_stream):
                    Yd = Y.to(self.device, non_blocking=True)
                    Cd = C.to(self.device, non_blocking=True)
                    Qd = Q.to(self.device, non_blocking=True)
                    ld = lab.to(self.device, non_blocking=True)
                copy_stream.synchronize()              # the pinned buffer goes back to the decoder ring after this
                for t in (Yd, Cd, Qd, ld):
                    t.record_stream(torch.cuda.current_stream(self.device))
                yield self._finish(Yd, Cd, Qd, ld)
        finally:
            stop.set()
            while th.is_alive():                        # drain so the producer can see `stop`
                try:
                    q.get_nowait()
                except queue.Empty:
                    pass
                th.join(timeout=0.05)

    def _finish(self, Y, C, Q, lab):
        if self.transform is None:
            return (Y, C, Q), lab
        return tuple(self.transform(Y, C, Q)), lab
