"""DCTBatchLoader(decode="device"): the producer finds the restart runs, the device walks them on a side stream, the transform gets
the same whole-grid tensors as from the host reader -- so both settings must yield equal tensors and labels, including for a file
the device path refuses (progressive), which arrives through the host reader."""
import pytest
import torch
from PIL import Image

import jpeg_cases as JC
import rgb_no_more_amd as rg
from rgb_no_more_amd import custom_transforms as CT
from rgb_no_more_amd.loader import DCTBatchLoader

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("jpeg_loader")
    paths = []
    for i in range(10):
        img = JC.noisy(512, 512, 40 + i, gray=(i == 6))
        p = d / f"s{i}.jpg"
        if i == 3:
            Image.fromarray(img).save(str(p), quality=90, subsampling="4:2:0", progressive=True)
        else:
            kw = {"restart_marker_rows": 1} if i % 2 else {}
            p.write_bytes(JC.encode(img, quality=90, **kw))
        paths.append(str(p))
    return paths, list(range(10))


def test_device_and_host_decode_yield_equal_batches(files):
    paths, labels = files
    ev = rg.datasets.get_transform("imagenet_dct", "val", dtype=torch.float32, fused=True)
    kw = dict(batch_size=4, device="cuda", threads=4, prefetch=2, shuffle=False, transform=ev)
    host = [(Y.clone(), C.clone(), lab.clone()) for (Y, C), lab in DCTBatchLoader(paths, labels, decode="host", **kw)]
    ld = DCTBatchLoader(paths, labels, decode="device", **kw)
    dev = [(Y.clone(), C.clone(), lab.clone()) for (Y, C), lab in ld]
    assert [b[2].tolist() for b in dev] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert len(host) == len(dev) == 3
    for (Yh, Ch, lh), (Yd, Cd, l_d) in zip(host, dev):
        assert torch.equal(lh, l_d) and torch.equal(Yh, Yd) and torch.equal(Ch, Cd)
    # what crossed PCIe for the last batch: compressed bytes and records, far below the 787 KB of coefficients per image
    assert 0 < ld.h2d_bytes < 2 * 400 * 1024
    # a second epoch re-uses the pinned ring
    again = [(Y.clone(), C.clone()) for (Y, C), _ in ld]
    for (Yh, Ch, _), (Yd, Cd) in zip(host, again):
        assert torch.equal(Yh, Yd) and torch.equal(Ch, Cd)


def test_raw_batches_without_a_transform(files):
    paths, labels = files
    a = [(Y.clone(), C.clone(), Q.clone()) for (Y, C, Q), _ in DCTBatchLoader(paths, labels, 5, device="cuda", shuffle=False, decode="host")]
    b = [(Y.clone(), C.clone(), Q.clone()) for (Y, C, Q), _ in DCTBatchLoader(paths, labels, 5, device="cuda", shuffle=False, decode="device")]
    for x, y in zip(a, b):
        for s, t in zip(x, y):
            assert s.dtype == torch.int16 and torch.equal(s, t)


def test_device_decode_excludes_crop_on_host(files):
    paths, labels = files
    tr = rg.datasets.get_transform("imagenet_dct", "train", ops_list=CT.VITTI_OPS, ops_magnitude=3, dtype=torch.float32, fused=True)
    with pytest.raises(ValueError, match="crop"):
        DCTBatchLoader(paths, labels, batch_size=4, device="cuda", transform=tr, crop_on_host=True, decode="device")
    with pytest.raises(ValueError):
        DCTBatchLoader(paths, labels, batch_size=4, device="cuda", decode="gpu")


def test_a_file_nobody_can_decode_raises_and_names_it(files, tmp_path):
    paths, labels = files
    bad = tmp_path / "broken.jpg"
    bad.write_bytes(b"this is not a jpeg file at all")
    with pytest.raises(Exception, match="broken.jpg"):
        for _ in DCTBatchLoader(paths[:3] + [str(bad)], labels[:4], batch_size=4, device="cuda", shuffle=False, decode="device"):
            pass
