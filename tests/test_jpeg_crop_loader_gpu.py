"""DCTBatchLoader(decode="device", crop_on_device=True): the producer draws the crop boxes before it prepares the plan, the device
walks and stores only the boxes, the transform reads them packed.  The yardstick is the host path with the same crop
(crop_on_host=True: libjpeg on the host, the same parameter sampler): both must yield equal tensors and labels at the same seed and
epoch, in fp32 and bf16, on files with a restart marker per MCU row, on files without markers, and with a progressive file in the
batch, which the device path hands to the host reader."""
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
    """name -> (paths, labels): 8 files of 512 x 512 (grid (64, 64)) each, two batches of 4.  "mixed": file 2 is progressive (the host
    fallback), file 5 gray."""
    d = tmp_path_factory.mktemp("jpeg_crop_loader")
    out = {}
    for name, kw in (("rows", {"restart_marker_rows": 1}), ("plain", {}), ("mixed", {"restart_marker_rows": 1})):
        paths = []
        for i in range(8):
            img = JC.noisy(512, 512, 60 + i, gray=(name == "mixed" and i == 5))
            p = d / f"{name}{i}.jpg"
            if name == "mixed" and i == 2:
                Image.fromarray(img).save(str(p), quality=90, subsampling="4:2:0", progressive=True)
            else:
                p.write_bytes(JC.encode(img, quality=90, **kw))
            paths.append(str(p))
        out[name] = (paths, list(range(10, 18)))
    return out


def batches(loader, epoch):
    loader.set_epoch(epoch)
    out = []
    for (Y, C), lab in loader:
        packed, nops = loader.last_packed
        out.append((Y.clone(), C.clone(), lab.clone(), packed.copy(), nops))
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["rows", "plain", "mixed"])
def test_crop_on_device_and_crop_on_host_yield_equal_batches(files, name, dtype):
    paths, labels = files[name]
    tr = rg.datasets.get_transform("imagenet_dct", "train", ops_list=CT.VITTI_OPS, ops_magnitude=3, dtype=dtype, fused=True)
    kw = dict(batch_size=4, device="cuda", threads=4, prefetch=2, shuffle=True, seed=7, transform=tr)
    host = DCTBatchLoader(paths, labels, crop_on_host=True, **kw)
    dev = DCTBatchLoader(paths, labels, decode="device", crop_on_device=True, **kw)
    for epoch in (0, 3):
        a, b = batches(host, epoch), batches(dev, epoch)
        assert len(a) == len(b) == 2
        for (Yh, Ch, lh, ph, nh), (Yd, Cd, l_d, pd, nd) in zip(a, b):
            assert Yd.dtype == dtype and Yd.is_cuda and tuple(Yd.shape)[:2] == (4, 1)
            assert torch.equal(lh, l_d) and nh == nd and ph.tobytes() == pd.tobytes()      # labels and last_packed
            assert torch.equal(Yh, Yd) and torch.equal(Ch, Cd)
    # what crossed PCIe for the last batch: compressed bytes, records and boxes, far below the crops' 380 KB per image
    assert 0 < dev.h2d_bytes < 4 * 200 * 1024
    first = batches(dev, 0)[0]
    assert not torch.equal(first[0], b[0][0])                    # another epoch, other boxes: the comparison above is not vacuous
