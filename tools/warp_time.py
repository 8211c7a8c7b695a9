#!/usr/bin/env python3
"""Dev tool (GPU box): what the batched warp chain (csrc/warp.hip, spnet_amd.augmentation.DeviceWarper) costs and what it
replaces.

  kernel     one spnet_warp_chain_u8 launch over 1,024 frames of 384x512 (uint8 out; also fp32 out), parameters drawn as
             the training draws them, against a plain device copy that moves the same bytes (1,024 x 196,608 read + as
             many written = 403 MB), buffers rotated beyond the Infinity Cache; median / min / max of 5 windows of 250 ms
  knockouts  (--knockouts) the same timing under diagnostic builds (-DSPNET_WARP_KO=bits, csrc/warp.hip)
  per image  the per-image path flip_image -> rotate_image -> translate_image (upload, three launches, download per step)
             over --images frames, in frames/s
  epoch      AugmentOnTheFly.on_epoch_begin over --frames written fake-ESPI files (331 layout), with and without warp,
             second call of each timed; the host time inside warp_targets is shown separately

usage: warp_time.py [--frames 4096] [--images 64] [--out profiles/warp_time.json] [--skip-epoch] [--knockouts]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tools.resize_time import gpu_time

KNOCKOUTS = ((1, "no global loads in the stage (constants to LDS)"), (2, "no global stores"), (3, "no loads, no stores"),
             (4, "one tap per pixel instead of four"), (7, "no loads, no stores, one tap (terms, box, LDS traffic, syncs)"),
             (8, "box never staged: every tap reads global memory"))


def draw_params(A, n, n_src, H, W, seed=0):
    state = np.random.get_state()
    np.random.seed(seed)
    p = A.new_warp_params([j % n_src for j in range(n)], H, W)
    for j in range(n):
        A.set_warp(p, j, *A.draw_warp(H, W))
    np.random.set_state(state)
    return p


def kernel_part(res):
    import torch
    from spnet_amd import _lib as L
    from spnet_amd import augmentation as A
    from spnet_amd import fake_espi as F
    N, H, W = 1024, 384, 512
    nrot = 3                                    # 3 x 403 MB: every launch reads and writes lines the caches no longer hold
    _, _, U = F.generate_device(N, seed=1, want_u8=True)
    U = U.reshape(N, H, W)
    src = [U.clone() for _ in range(nrot)]
    outu = [torch.empty((N, H, W), dtype=torch.uint8, device="cuda") for _ in range(nrot)]
    outf = torch.empty((N, H, W), dtype=torch.float32, device="cuda")
    p = draw_params(A, N, N, H, W)
    rec = np.zeros(N, A.WARP_RECORD)
    rec["m"], rec["flip"], rec["xt"], rec["yt"] = p["minv"], p["flip"], p["xt"], p["yt"]
    recd = torch.from_numpy(rec.view(np.int32).reshape(-1).copy()).cuda()
    sel = torch.from_numpy(p["index"]).cuda()
    st = L.current_stream()

    def launch(i, u, f):
        L.spnet_warp_chain_u8(src[i].data_ptr(), N, sel.data_ptr(), recd.data_ptr(), N, H, W, u, f, st)

    t_copy = gpu_time(lambda i: outu[i].copy_(src[i]), nrot)
    t_u = gpu_time(lambda i: launch(i, outu[i].data_ptr(), None), nrot)
    t_f = gpu_time(lambda i: launch(i, None, outf.data_ptr()), nrot)
    nbytes = 2 * N * H * W
    res["kernel"] = {"frames": N, "bytes_u8_out": nbytes, "copy_same_bytes": t_copy, "warp_u8": t_u, "warp_fp32": t_f,
                     "ratio_to_copy": t_u["us"] / t_copy["us"], "frames_per_s_u8": N / (t_u["us"] * 1e-6),
                     "TB_per_s_u8": nbytes / (t_u["us"] * 1e-6) / 1e12, "library": os.path.basename(L.LIB_PATH)}
    print("kernel [%s]: 1,024 frames -> uint8 %.1f us (%.1f-%.1f; %.2f TB/s, %.0f frames/s), fp32 %.1f us; copy of the same "
          "bytes %.1f us (%.1f-%.1f) (x%.2f)"
          % (os.path.basename(L.LIB_PATH), t_u["us"], t_u["min_us"], t_u["max_us"], nbytes / t_u["us"] / 1e6,
             N / (t_u["us"] * 1e-6), t_f["us"], t_copy["us"], t_copy["min_us"], t_copy["max_us"], t_u["us"] / t_copy["us"]),
          flush=True)


def knockout_part(res):
    """The kernel timing under diagnostic builds of the library, each in a fresh process with SPNET_HIP_LIB; a variant
    library that is not there yet is built first."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = []
    for bits, what in KNOCKOUTS:
        lib = os.path.join(root, "tools", "libwarp_ko%d.so" % bits)
        if not os.path.exists(lib):
            subprocess.run(["bash", os.path.join(root, "tools", "build_variant_lib.sh"), "warp_ko%d" % bits,
                            "-DSPNET_WARP_KO=%d" % bits], check=True)
        tmp = tempfile.NamedTemporaryFile(suffix=".json", delete=False).name
        subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-only", "--out", tmp],
                       env=dict(os.environ, SPNET_HIP_LIB=lib), check=True, timeout=120, stdout=subprocess.DEVNULL)
        k = json.load(open(tmp))["kernel"]
        os.remove(tmp)
        rows.append({"bits": bits, "what": what, "warp_u8_us": k["warp_u8"]["us"], "warp_fp32_us": k["warp_fp32"]["us"],
                     "copy_us": k["copy_same_bytes"]["us"]})
        print("knock-out %2d  uint8 %7.1f us  fp32 %7.1f us  (copy %.1f)  %s"
              % (bits, k["warp_u8"]["us"], k["warp_fp32"]["us"], k["copy_same_bytes"]["us"], what), flush=True)
    res["knockouts"] = rows


def per_image_part(res, n):
    """The per-image functions: every step uploads the image as fp32, launches and downloads it again."""
    import torch
    from spnet_amd import augmentation as A
    from spnet_amd import fake_espi as F
    _, _, U = F.generate_device(n, seed=2, want_u8=True)
    X = U.reshape(n, 384, 512).cpu().numpy()
    imgs = [np.repeat(x[..., None], 3, axis=2) for x in X]
    state = np.random.get_state()

    def run():
        np.random.seed(0)
        for img in imgs:
            a, _, _ = A.flip_image(img, [], "f", int(np.random.choice([-2, -1, 0, 1])))
            a, _, _ = A.rotate_image(a, [], "f", np.random.uniform(-20, high=20))
            A.translate_image(a, [], "f", np.random.randint(10))
        torch.cuda.synchronize()
    run()
    t = []
    for _ in range(3):
        t0 = time.time()
        run()
        t.append(time.time() - t0)
    np.random.set_state(state)
    t.sort()
    res["per_image"] = {"images": n, "channels": 3, "seconds": t[1], "frames_per_s": n / t[1]}
    print("per image (flip_image -> rotate_image -> translate_image, 3-channel uint8): %.0f frames/s" % (n / t[1]), flush=True)


def epoch_part(res, n):
    import torch
    from spnet_amd import callbacks as C
    from spnet_amd import fake_espi as F
    from spnet_amd import utils
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "Train")
        F.write_dataset(path, n, seed=3)
        X, Y, files, _ = utils.build_dataset(path=path + "/", shuffle=False)
        Xd = torch.from_numpy(X).cuda()
        out = {}
        for warp in (False, True):
            cb = C.AugmentOnTheFly(Xd, Y, warp=warp, warp_files=list(files) if warp else None)
            t = []
            for e in range(3):
                torch.cuda.synchronize()
                t0 = time.time()
                cb.on_epoch_begin(e)
                torch.cuda.synchronize()
                t.append(time.time() - t0)
            out["warp" if warp else "plain"] = {"seconds": min(t[1:]), "first_call_seconds": t[0]}
            if warp:
                out["warp"]["host_label_seconds"] = cb.label_seconds
                out["warp"]["rejected_last_epoch"] = cb.rejected
            del cb
    out["frames"] = n
    res["epoch_begin"] = out
    print("epoch begin over %d frames: plain %.3f s, with warp %.3f s (host labels %.3f s of it)"
          % (n, out["plain"]["seconds"], out["warp"]["seconds"], out["warp"]["host_label_seconds"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default="profiles/warp_time.json")
    ap.add_argument("--skip-epoch", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--knockouts", action="store_true", help="also time the kernel under the diagnostic knock-out builds")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "warp_time.py measures on the GPU"
    res = {"device": torch.cuda.get_device_name(0)}
    kernel_part(res)
    if args.knockouts:
        knockout_part(res)
    if not args.kernel_only:
        per_image_part(res, args.images)
        if not args.skip_epoch:
            epoch_part(res, args.frames)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
