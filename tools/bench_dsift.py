"""Dense-SIFT producer throughput (csrc/pxr_dsift.hip).  One JSON line on stdout; --out FILE also writes it.

    python tools/bench_dsift.py [--out FILE] [--kernel-trace DIR] [--quick]

Shapes a user runs (BASELINE configs[0] / configs[1]):
  c0  10 grey images of 2000 x 1500 (dsift.yaml's max_edge 2000), 2000 keypoints each
  c1  1000 grey images of 2000 x 1500, 100 keypoints each (100k keypoints)
Per shape, timed with device events after a warm-up (all inputs resident on the device, launches through the C-ABI):
  fused       pxr_dsift_extract per image into one fp16 arena (16 x 16 patches, 128 channels)
  dense       pxr_dsift_dense per image into a 128 x h x w fp32 map, then pxr_arena_extract
  torch_ref   the reference's way on the same GPU: the torch-ROCm composition of kornia's DenseSIFTDescriptor in fp32
              (F.pad + conv2d gradient, outer-product pooling conv2d, identity gather conv2d, F.normalize) + F.normalize of
              the extractor, then pxr_arena_extract (c1: on the first `torch_images` images, per-image figure scaled)
and end to end on c0-shaped JPEG files: features_from_image_list(device=True) wall time, with the PIL decode + grey
conversion (FeatureExtractor.preprocess) timed on its own.
--kernel-trace DIR: a `rocprofv3 --kernel-trace --stats` run of this script (a run of its own; --quick has the same launch
shapes) -> kernel-only times: the median launch of each kernel at each shape's grid x the launches of a pass.
"""
import argparse
import csv
import glob
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

PEAK_HBM = 8.0e12
PS, CH = 16, 128


def torch_dsift(x, s=4, clipval=0.2):
    """(1, 1, h, w) fp32 cuda -> (1, 128, h, w): kornia's composition in torch ops (the reference's dsift model)."""
    import torch
    import torch.nn.functional as F
    h, w = x.shape[2:]
    xp = F.pad(x, (1, 1, 1, 1), mode="replicate")
    kx = torch.tensor([[0.0, 0.0, 0.0], [-0.5, 0.0, 0.5], [0.0, 0.0, 0.0]], device=x.device)
    gx = F.conv2d(xp, kx[None, None])
    gy = F.conv2d(xp, kx.t().contiguous()[None, None])
    mag = torch.sqrt(gx * gx + gy * gy + 1e-10)
    o = 8.0 * (torch.atan2(gy, gx + 1e-10) + 2.0 * math.pi) / (2.0 * math.pi)
    f = torch.floor(o)
    w1 = o - f
    b0 = torch.remainder(f, 8)
    b1 = torch.remainder(b0 + 1, 8)
    A = torch.cat([(b0 == a).float() * (1.0 - w1) * mag + (b1 == a).float() * w1 * mag for a in range(8)], 1)
    hs = s / 2.0
    k = torch.tensor([(hs - abs(i + 0.5 - hs)) / hs for i in range(s)], device=x.device)
    P = F.conv2d(A.view(8, 1, h, w), torch.outer(k, k)[None, None], padding=s // 2).view(1, 8, h + 1, w + 1)
    D = F.conv2d(P, torch.eye(128, device=x.device).view(128, 8, 4, 4), padding=1)
    out = F.normalize(D, dim=1).clamp_(0.0, clipval)
    out = F.normalize(out, dim=1)
    return torch.sqrt(F.normalize(out, dim=1, p=1) + 1e-10)


def kernel_times(d):
    """{(kernel, grid size): [durations in ms]} of the dsift / extract kernels from a rocprofv3 --kernel-trace run."""
    out = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row["Kernel_Name"]
            key = next((k for k in ("dsift_extract_kernel", "dsift_dense_kernel", "extract_kernel") if k in name), None)
            if key is None:
                continue
            grid = int(row.get("Grid_Size_X", row.get("Grid_Size", 0)) or 0)
            out.setdefault((key, grid), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    return out


def kernel_summary(res, d, shapes):
    """Kernel-only figures per shape: the median launch of each kernel at the shape's grid x the launches per pass."""
    kt = kernel_times(d)
    res["kernel_trace"] = {"%s grid %d" % k: {"launches": len(v), "median_ms": float(np.median(v))} for k, v in sorted(kt.items())}
    for tag, (n_img, per) in shapes.items():
        f = kt.get(("dsift_extract_kernel", per * 256))
        if not f or tag not in res:
            continue
        r = res[tag]
        ms = float(np.median(f)) * n_img
        r["fused_kernel_ms"] = ms
        r["fused_kernel_keypoints_per_s"] = r["keypoints"] / (ms * 1e-3)
        r["fused_kernel_write_share_of_8TBs"] = r["written_bytes"] / (ms * 1e-3) / PEAK_HBM
        dn, ex = kt.get(("dsift_dense_kernel", 0)), kt.get(("extract_kernel", per * 256))
        dn = dn or next((v for (k, g), v in kt.items() if k == "dsift_dense_kernel"), None)
        if dn and ex:
            r["dense_kernel_ms"] = float(np.median(dn)) * n_img
            r["dense_extract_kernel_ms"] = float(np.median(ex)) * n_img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--kernel-trace", help="directory of a rocprofv3 --kernel-trace run of this script")
    ap.add_argument("--quick", action="store_true", help="small sizes (the profiled run / rehearsal)")
    args = ap.parse_args()
    import torch
    from pixsfm_amd._lib import F32, U8, check
    from pixsfm_amd.engine import Context, PatchArena
    ctx = Context(0)
    lib = ctx.lib
    dev = "cuda:0"
    H, W = (1500, 2000)
    shapes = {"c0": (10, 2000), "c1": (1000, 100)}
    torch_images = 20
    if args.quick:
        shapes = {"c0": (2, 2000), "c1": (40, 100)}
        torch_images = 2
    res = {"tool": "tools/bench_dsift.py", "image": [W, H], "patch": [PS, PS, CH], "arena_dtype": "float16",
           "spatial_bin_size": 4, "rootsift": True, "quick": bool(args.quick)}
    gen = torch.Generator(device=dev).manual_seed(0)

    def timed(fn, reps):
        fn()
        ctx.sync()
        torch.cuda.synchronize()
        ctx.timer_start()
        for _ in range(reps):
            fn()
        return ctx.timer_stop() / reps

    for tag, (n_img, per) in shapes.items():
        imgs = torch.randint(0, 256, (n_img, H, W), dtype=torch.uint8, device=dev, generator=gen)
        n = n_img * per
        rng = np.random.default_rng(1)
        kp = rng.uniform([0, 0], [W, H], (n, 2))
        d_kp = ctx.to_device(kp, np.float64)
        torch.cuda.synchronize()
        arena = PatchArena(ctx, n, PS, PS, CH, np.float16)
        kp_ptr = d_kp.ptr.value

        def fused():
            for i in range(n_img):
                check(lib.pxr_dsift_extract(ctx.handle, arena.handle, i * per, per, C.c_void_p(imgs[i].data_ptr()), U8, H, W,
                                            4, 1, 0.2, C.c_void_p(kp_ptr + 16 * i * per), float(W), float(H), 1),
                      "pxr_dsift_extract")
        ms = timed(fused, 3 if not args.quick else 1)
        out_bytes = n * PS * PS * CH * 2
        r = {"images": n_img, "keypoints": n, "fused_ms": ms, "fused_keypoints_per_s": n / (ms * 1e-3),
             "written_bytes": out_bytes, "fused_write_share_of_8TBs": out_bytes / (ms * 1e-3) / PEAK_HBM}
        fused_patches = arena.download(0, min(n, 64))[0]
        dmap = torch.empty((CH, H, W), dtype=torch.float32, device=dev)
        arena2 = PatchArena(ctx, n, PS, PS, CH, np.float16)

        def dense(count=n_img):
            for i in range(count):
                check(lib.pxr_dsift_dense(ctx.handle, C.c_void_p(imgs[i].data_ptr()), U8, H, W, 4, 1, 0.2,
                                          C.c_void_p(dmap.data_ptr())), "pxr_dsift_dense")
                check(lib.pxr_arena_extract(ctx.handle, arena2.handle, i * per, per, C.c_void_p(dmap.data_ptr()), F32, H, W,
                                            C.c_void_p(kp_ptr + 16 * i * per), float(W), float(H), 1), "pxr_arena_extract")
        ms_d = timed(dense, 1)
        r["dense_then_extract_ms"] = ms_d
        r["dense_equals_fused_bitwise"] = bool(np.array_equal(arena2.download(0, min(n, 64))[0].view(np.int16),
                                                              fused_patches.view(np.int16)))
        # the reference's way: torch composition in fp32 + the extractor's F.normalize + the existing extract
        nt = min(n_img, torch_images)
        ctx.sync()

        def torch_way():
            for i in range(nt):
                x = imgs[i].float().div_(255.0)[None, None]
                fm = torch.nn.functional.normalize(torch_dsift(x), dim=1).contiguous()
                torch.cuda.current_stream().synchronize()
                check(lib.pxr_arena_extract(ctx.handle, arena2.handle, i * per, per, C.c_void_p(fm.data_ptr()), F32, H, W,
                                            C.c_void_p(kp_ptr + 16 * i * per), float(W), float(H), 1), "pxr_arena_extract")
                ctx.sync()
        torch_way()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch_way()
        torch.cuda.synchronize()
        ms_t = (time.perf_counter() - t0) * 1e3
        r["torch_ref_images_timed"] = nt
        r["torch_ref_ms"] = ms_t * n_img / nt
        r["torch_ref_note"] = "host clock around synchronised work" + ("" if nt == n_img else ", per-image time x %d" % n_img)
        tp = arena2.download(0, min(per, 64))[0].astype(np.float32)
        r["torch_ref_vs_fused_max_abs"] = float(np.abs(tp - fused_patches[:len(tp)].astype(np.float32)).max())
        r["fused_speedup_vs_dense"] = ms_d / ms
        r["fused_speedup_vs_torch_ref"] = r["torch_ref_ms"] / ms
        res[tag] = r
        arena.close(); arena2.close()
        del imgs, dmap
        torch.cuda.empty_cache()

    # end to end on c0-shaped JPEG files
    from PIL import Image
    from pixsfm_amd.api import FeatureExtractor, features_from_image_list
    n_img, per = shapes["c0"]
    with tempfile.TemporaryDirectory() as d:
        rng = np.random.default_rng(2)
        yy, xx = np.mgrid[0:H, 0:W]
        base = 127 + 80 * np.sin(xx / 9.0) * np.cos(yy / 7.0)
        names, kps = [], {}
        for i in range(n_img):
            rgb = np.clip(base[..., None] + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8)
            name = "img%03d.jpg" % i
            Image.fromarray(rgb).save(os.path.join(d, name), quality=90)
            names.append(name)
            kps[name] = rng.uniform([0, 0], [W, H], (per, 2))
        ex = FeatureExtractor({"model": {"name": "dsift", "rootsift": True, "spatial_bin_size": 4}, "max_edge": 2000,
                               "patch_size": PS, "device": "cuda"}, ctx=ctx)
        features_from_image_list(ex, d, names[:1], keypoints={names[0]: kps[names[0]]}, device=True)   # warm-up
        t0 = time.perf_counter()
        for name in names:
            ex.preprocess(os.path.join(d, name))
        t_pre = time.perf_counter() - t0
        t0 = time.perf_counter()
        fm = features_from_image_list(ex, d, names, keypoints=kps, device=True)
        ctx.sync()
        t_all = time.perf_counter() - t0
        res["e2e_c0"] = {"images": n_img, "keypoints": n_img * per, "features_from_image_list_s": t_all,
                         "pil_decode_and_grey_s": t_pre, "rest_s": t_all - t_pre,
                         "note": "JPEG quality 90, 2000 x 1500 RGB; max_edge 2000 (no resize); device=True: one fp16 arena"}
        fm.fset(0).arena.close()
    if args.kernel_trace:
        kernel_summary(res, args.kernel_trace, shapes)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
