"""What the crop form of the device JPEG decode (rgbnm_jpeg_decode_batch_crop) must do, restated in numpy for its tests: how many
MCUs the lane of a run walks for a crop box, the boxes the tests try on a grid, and the box cut out of whole-grid tensors in the
packed layout.  A plain module, imported by name."""
import numpy as np
import torch

S420, GRAY = [(2, 2), (1, 1), (1, 1)], [(1, 1)]


def expected_walked(mcu0, nmcu, mcus_x, sampling, box):
    """MCUs the lane of run [mcu0, mcu0 + nmcu) walks: up to the run's last MCU, in raster order, that holds a block inside its
    component's box; 0 if it holds none.  sampling: (hs, vs) per component ([(1, 1)] for a one-component file, whose MCU is one
    block); box: (top, left, h, w) in luma blocks, halved for components 1 and 2.  Every MCU of the run is looked at."""
    m = np.arange(mcu0, mcu0 + nmcu)
    mx, my = m % mcus_x, m // mcus_x
    need = np.zeros(nmcu, dtype=bool)
    for c, (hs, vs) in enumerate(sampling):
        t, l, h, w = [int(v) // 2 for v in box] if c else [int(v) for v in box]
        need |= (mx * hs < l + w) & (mx * hs + hs > l) & (my * vs < t + h) & (my * vs + vs > t)
    idx = np.nonzero(need)[0]
    return int(idx[-1]) + 1 if idx.size else 0


def plan_walked(plan, boxes):
    """expected_walked for every run record of a prepared plan (dct_manip.JpegBatchPlan): int32 [nruns]."""
    runs, images = plan.runs[:plan.nruns].numpy(), plan.images[:plan.n].numpy()
    out = np.zeros(plan.nruns, dtype=np.int32)
    for ri, r in enumerate(runs):
        image, mcu0, nmcu = int(r[2]), int(r[3]), int(r[4])
        if nmcu == 0:
            continue
        im = images[image]
        ncomp, mcus_x = int(im[0]), int(im[1])
        sampling = [(int(im[11 + c]), int(im[14 + c])) for c in range(ncomp)]          # hs at 11..13, vs at 14..16 (rgbnm_jpeg_image)
        out[ri] = expected_walked(mcu0, nmcu, mcus_x, sampling, boxes[image])
    return out


def boxes_for(grid):
    """name -> (top, left, h, w) on a luma grid: the largest even box (on an odd grid it ends at the last even row and column, so the
    padding blocks fall outside), 2 x 2 boxes at the corners and in the middle, one MCU row at full width, one MCU column at full height."""
    hb, wb = grid
    he, we = hb & ~1, wb & ~1
    mid = (he // 2 & ~1, we // 2 & ~1)
    return {"largest": (0, 0, he, we), "top_left": (0, 0, 2, 2), "top_right": (0, we - 2, 2, 2), "bottom_left": (he - 2, 0, 2, 2),
            "bottom_right": (he - 2, we - 2, 2, 2), "middle": (mid[0], mid[1], 2, 2), "mcu_row": (mid[0], 0, 2, we),
            "mcu_column": (0, mid[1], he, 2)}


def cut(Y, C, boxes):
    """The boxes cut out of whole-grid tensors Y [n, 1, Hb, Wb, 8, 8], C [n, 2, Hbc, Wbc, 8, 8], packed back to back as
    read_coefficients_batch_crop packs them: (Ypacked, Cpacked) flat."""
    ys, cs = [], []
    for i, (t, l, h, w) in enumerate(np.asarray(boxes).tolist()):
        ys.append(Y[i, 0, t:t + h, l:l + w].reshape(-1))
        cs.append(C[i, :, t // 2:(t + h) // 2, l // 2:(l + w) // 2].reshape(-1))
    return torch.cat(ys), torch.cat(cs)
