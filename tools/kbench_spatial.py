"""`spatial_pair` (csrc/spatial/spatial.hip) at the training shape against its byte floor, the numpy restatement, and the whole of
`augment_frames` against the host path it replaces.

    python tools/kbench_spatial.py [--out profiles/spatial_kbench.json]

Rows: B = 4 frames of 540 x 960 with the parameters `draw_spatial` gives.  The `*WoCrop` form crops (160 s) x (320 s) at the scales
1.0 / 1.65 / 2.3 / 2.95 and resizes the images to 160 x 320 (uint8 -> fp32, what `augment_frames` runs; dense and sparse); the
fixed-crop form crops 320 x 720 without final resize (uint8 -> uint8).

`entry_us` = device events around repeated warm calls of `spt_spatial_pair` alone on preallocated outputs; `op_us` = the same around
the Python op (allocations, parameter table and ctypes call included); median of the blocks.  `floor_us` = (outputs written once +
the source footprint read once) at the bandwidth the other kbench files use, the footprint being the source rectangle behind each
crop: crop area / (scale_x scale_y) pixels of both images and of the ground truth.  `host_us` = `spatial_pair_host` on CPU tensors plus
the upload of its result, host clock, best of 2.  `frames_us` / `frames_host_us`: `augment_frames` (photometric, eraser, spatial,
final resize) on the device, and `photometric_pair_host` + `spatial_pair_host` + upload.  Nothing is asserted on these numbers.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "any-stereo_amd")]

HBM_BPS = 6.3e12
SCALES = (1.0, 1.65, 2.3, 2.95)


def _events(fn, reps, blocks):
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e3)
    return sorted(out)[len(out) // 2]


def _best(fn, n=2):
    best = None
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e6
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from anystereo import _spatial_lib as L, ops
    from anystereo.harness import augment as A, spatial as SP
    assert torch.cuda.is_available(), "kbench_spatial needs a GPU"
    dev = torch.device("cuda:0")
    bsz, h, w, lr = 4, 540, 960, (160, 320)
    g = torch.Generator().manual_seed(1)
    u1 = torch.randint(0, 256, (bsz, 3, h, w), generator=g, dtype=torch.uint8)
    u2 = torch.randint(0, 256, (bsz, 3, h, w), generator=g, dtype=torch.uint8)
    disp = torch.rand((bsz, h, w), generator=g) * 200 + 1
    valid = (torch.rand((bsz, h, w), generator=g) < 0.3).to(torch.uint8)
    d1, d2, dd, dv = u1.to(dev), u2.to(dev), disp.to(dev), valid.to(dev)
    ragged = [(round(lr[0] * s), round(lr[1] * s)) for s in SCALES]
    rows = []
    for label, spec, sizes, out_size, out_dtype, sparse in (
            ("WoCrop dense u8->f32 LR 160x320", SP.SpatialSpec.flow(), ragged, lr, torch.float32, False),
            ("WoCrop sparse u8->f32 LR 160x320", SP.SpatialSpec.sparse(wo_crop=True), ragged, lr, torch.float32, True),
            ("fixed crop 320x720 dense u8->u8", SP.SpatialSpec.flow(), [(320, 720)] * bsz, None, torch.uint8, False)):
        params = SP.draw_spatial(spec, 1, 0, bsz, h, w, sizes)
        hv, gv = (valid, dv) if sparse else (None, None)
        h_out, w_out = out_size if out_size else sizes[0]
        es = 4 if out_dtype == torch.float32 else 1
        out_bytes = 2 * bsz * 3 * h_out * w_out * es + sum(ch * cw * (5 if sparse else 4) for ch, cw in sizes)
        src_px = sum(p.ch * p.cw / (p.scale_x * p.scale_y) for p in params)
        in_bytes = int(src_px * (6 + 4 + (1 if sparse else 0)))
        floor = (out_bytes + in_bytes) / HBM_BPS * 1e6
        op_us = _events(lambda: SP.spatial_pair(d1, d2, dd, params, valid=gv, out_size=out_size, out_dtype=out_dtype), a.reps, a.blocks)
        got = SP.spatial_pair(d1, d2, dd, params, valid=gv, out_size=out_size, out_dtype=out_dtype)
        # the C entry alone, on the outputs of the call above
        table = SP.c_samples(params)
        dptr = (C.c_void_p * bsz)(*[t.data_ptr() for t in got[2]])
        vptr = None if not sparse else (C.c_void_p * bsz)(*[t.data_ptr() for t in got[3]])
        lib, stream = L.load(), ops._stream()
        oh, ow = out_size if out_size else (0, 0)
        args = (ops._p(d1), ops._p(d2), 0, ops._p(dd), ops._p(gv), bsz, h, w, table, ops._p(got[0]), ops._p(got[1]), 1 if es == 4 else 0, oh, ow,
                dptr, vptr, stream)
        assert lib.spt_spatial_pair(*args) == 0
        entry_us = _events(lambda: lib.spt_spatial_pair(*args), a.reps, a.blocks)
        want = SP.spatial_pair_host(u1, u2, disp, params, valid=hv, out_size=out_size, out_dtype=out_dtype)
        same = (torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
                and all(torch.equal(x.cpu().view(torch.int32), y.view(torch.int32)) for x, y in zip(got[2], want[2]))
                and (not sparse or all(torch.equal(x.cpu(), y) for x, y in zip(got[3], want[3]))))

        def host():
            o = SP.spatial_pair_host(u1, u2, disp, params, valid=hv, out_size=out_size, out_dtype=out_dtype)
            for t in [o[0], o[1]] + o[2] + (o[3] or []):
                t.to(dev)
            torch.cuda.synchronize()
        row = {"row": label, "B": bsz, "frame": [h, w], "crops": [list(s) for s in sizes], "out_size": list(out_size) if out_size else None,
               "scales_xy": [[round(p.scale_x, 4), round(p.scale_y, 4)] for p in params], "flips": [p.flip for p in params],
               "bytes_out": out_bytes, "bytes_source_footprint": in_bytes, "launches": 2, "floor_us": round(floor, 2),
               "entry_us": round(entry_us, 2), "op_us": round(op_us, 2), "entry_of_floor": round(floor / entry_us, 4),
               "host_us": round(_best(host), 0), "equal_to_host": bool(same)}
        rows.append(row)
        print(json.dumps(row), flush=True)

    # the whole of augment_frames against the host path it replaces
    photo, spec = A.PhotoSpec.flow(), SP.SpatialSpec.flow()
    frames_us = _events(lambda: SP.augment_frames(d1, d2, dd, photo, spec, 1, 0, SCALES, lr), max(a.reps // 5, 5), a.blocks)

    def frames_host():
        o = SP.augment_frames(u1, u2, disp, photo, spec, 1, 0, SCALES, lr)
        for t in [o[0], o[1]] + o[2]:
            t.to(dev)
        torch.cuda.synchronize()
    frames = {"row": "augment_frames flow B=4 540x960 -> LR 160x320", "frames_us": round(frames_us, 2), "frames_host_us": round(_best(frames_host), 0)}
    print(json.dumps(frames), flush=True)
    result = {"tool": "kbench_spatial", "command": "python tools/kbench_spatial.py --reps %d --blocks %d" % (a.reps, a.blocks),
              "device": torch.cuda.get_device_name(0), "library": L.library_info(), "hbm_tb_s": HBM_BPS / 1e12, "rows": rows, "augment_frames": frames}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
