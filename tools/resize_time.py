#!/usr/bin/env python3
"""Dev tool (GPU box): what the device resize (csrc/resize.hip, spnet_amd/resize.py) costs and what it replaces.

  kernel    one spnet_resize_u8 launch, 128 frames 384x512 -> 331x331, fp32 output (also uint8 only / both), against a
            plain device copy that moves the same bytes (128 x (196,608 read + 438,244 written) = 81 MB), buffers
            rotated beyond the Infinity Cache; median / min / max of 5 windows of 250 ms of back-to-back launches
  knockouts (--knockouts) the same timing under diagnostic builds of the library that leave out the HBM loads, the HBM
            stores, the taps of either pass, the exact division (-DSPNET_RESIZE_KO=bits, csrc/resize.hip): where the
            launch's time goes
  loading   build_X over --files written PNGs: the parent's way (force_dim=331, as_uint8: decode + PIL resize per frame)
            against device_resize=True (decode only), and the PIL resize alone on already decoded frames
  predict   predict_network wall time on those files, host resize against --device_resize (same model), and
            Model.predict alone on the loaded frames (second call of each timed: plans and rings exist)

usage: resize_time.py [--files 2048] [--out profiles/resize_time.json] [--skip-files] [--knockouts]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


KNOCKOUTS = ((1, "no HBM loads (stage writes constants to LDS)"), (2, "no HBM stores"), (3, "no HBM loads, no stores"),
             (4, "horizontal pass: 1 tap per output instead of 12"), (8, "vertical pass: 1 tap per output"),
             (12, "both passes 1 tap"), (16, "network-input conversion without the exact division"),
             (28, "both passes 1 tap, no division"), (31, "everything knocked out (launch, staging, LDS traffic, syncs)"))


def gpu_time(fn, nrot, window_ms=250.0, repeats=5):
    """Median / min / max over `repeats` windows of about window_ms of back-to-back launches, in us per launch."""
    import torch

    def window(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i % nrot)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    for i in range(3):
        fn(i % nrot)
    torch.cuda.synchronize()
    iters = max(30, int(window_ms * 1e3 / max(window(30), 1.0)))
    t = sorted(window(iters) for _ in range(repeats))
    return {"us": t[len(t) // 2], "min_us": t[0], "max_us": t[-1], "launches_per_window": iters, "windows": repeats}


def kernel_part(res):
    """The raw entry point (no Python wrapper between launches) and a plain device copy of the same bytes."""
    import torch
    from spnet_amd import _lib as L
    from spnet_amd import fake_espi as F
    from spnet_amd import resize as RZ
    N, H, W, O = 128, 384, 512, 331
    nrot = 12                                   # 12 x 81 MB: every launch reads and writes cold lines
    _, _, U = F.generate_device(N, seed=1, want_u8=True)
    src = [U.clone() for _ in range(nrot)]
    outf = [torch.empty((N, O, O, 1), device="cuda") for _ in range(nrot)]
    outu = [torch.empty((N, O, O), dtype=torch.uint8, device="cuda") for _ in range(nrot)]
    nbytes = N * (H * W + O * O * 4)
    cp_a = [torch.empty(nbytes // 2 // 16 * 16, dtype=torch.uint8, device="cuda") for _ in range(nrot)]
    cp_b = [torch.empty_like(cp_a[0]) for _ in range(nrot)]
    (xt, xtaps), (yt, ytaps) = RZ.warm(W, O, "cuda:0"), RZ.warm(H, O, "cuda:0")
    st = L.current_stream()
    sp, fp, up = [t.data_ptr() for t in src], [t.data_ptr() for t in outf], [t.data_ptr() for t in outu]
    xp, yp = xt.data_ptr(), yt.data_ptr()

    def launch(i, f, u):
        L.spnet_resize_u8(sp[i], N, H, W, xp, xtaps, yp, ytaps, O, O, u, f, st)

    t_copy = gpu_time(lambda i: cp_b[i].copy_(cp_a[i]), nrot)
    t_f = gpu_time(lambda i: launch(i, fp[i], None), nrot)
    t_u = gpu_time(lambda i: launch(i, None, up[i]), nrot)
    t_b = gpu_time(lambda i: launch(i, fp[i], up[i]), nrot)
    res["kernel"] = {"frames": N, "bytes_fp32_out": nbytes, "copy_same_bytes": t_copy, "resize_fp32": t_f,
                     "resize_u8": t_u, "resize_both": t_b, "ratio_to_copy": t_f["us"] / t_copy["us"],
                     "frames_per_s_fp32": N / (t_f["us"] * 1e-6), "TB_per_s_fp32": nbytes / (t_f["us"] * 1e-6) / 1e12,
                     "library": os.path.basename(L.LIB_PATH)}
    print("kernel [%s]: 128 frames -> fp32 %.1f us (%.1f-%.1f; %.2f TB/s, %.0f frames/s), uint8 %.1f us, both %.1f us; "
          "copy of the same bytes %.1f us (%.1f-%.1f) (x%.2f)"
          % (os.path.basename(L.LIB_PATH), t_f["us"], t_f["min_us"], t_f["max_us"], nbytes / t_f["us"] / 1e6,
             N / (t_f["us"] * 1e-6), t_u["us"], t_b["us"], t_copy["us"], t_copy["min_us"], t_copy["max_us"],
             t_f["us"] / t_copy["us"]), flush=True)


def knockout_part(res):
    """The same kernel timing under diagnostic builds of the library (-DSPNET_RESIZE_KO=bits, csrc/resize.hip), each in a
    fresh process with SPNET_HIP_LIB; a variant library that is not there yet is built first."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = []
    for bits, what in KNOCKOUTS:
        lib = os.path.join(root, "tools", "libresize_ko%d.so" % bits)
        if not os.path.exists(lib):
            subprocess.run(["bash", os.path.join(root, "tools", "build_variant_lib.sh"), "resize_ko%d" % bits,
                            "-DSPNET_RESIZE_KO=%d" % bits], check=True)
        tmp = tempfile.NamedTemporaryFile(suffix=".json", delete=False).name
        subprocess.run([sys.executable, os.path.abspath(__file__), "--skip-files", "--out", tmp],
                       env=dict(os.environ, SPNET_HIP_LIB=lib), check=True, timeout=120, stdout=subprocess.DEVNULL)
        k = json.load(open(tmp))["kernel"]
        os.remove(tmp)
        rows.append({"bits": bits, "what": what, "resize_fp32_us": k["resize_fp32"]["us"],
                     "resize_u8_us": k["resize_u8"]["us"], "copy_us": k["copy_same_bytes"]["us"]})
        print("knock-out %2d  fp32 %6.1f us  uint8 %6.1f us  (copy %.1f)  %s"
              % (bits, k["resize_fp32"]["us"], k["resize_u8"]["us"], k["copy_same_bytes"]["us"], what), flush=True)
    res["knockouts"] = rows


def wall(fn, repeats=5):
    t = []
    for _ in range(repeats):
        t0 = time.time()
        fn()
        t.append(time.time() - t0)
    t.sort()
    return {"s": t[len(t) // 2], "min_s": t[0], "max_s": t[-1], "repeats": repeats}


def files_part(res, nfiles):
    import glob
    from PIL import Image
    import predict_spnet
    from spnet_amd import fake_espi as F
    from spnet_amd import models as M
    from spnet_amd import utils as U
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "frames") + "/"
        F.write_dataset(path, nfiles, seed=11)
        files = sorted(glob.glob(path + "*.png"))
        t0 = time.time()
        X_host, _ = U.build_X(nfiles, files, force_dim=331, grayscale=True, as_uint8=True)
        t_host = time.time() - t0
        t0 = time.time()
        X_nat, _ = U.build_X(nfiles, files, force_dim=331, grayscale=True, as_uint8=True, device_resize=True)
        t_nat = time.time() - t0
        t0 = time.time()                        # the PIL resize alone, one process (build_X spreads it over a pool)
        for a in X_nat[:256, :, :, 0]:
            Image.fromarray(a).convert("RGB").resize((331, 331), Image.LANCZOS)
        t_pil = (time.time() - t0) / 256
        res["loading"] = {"files": nfiles, "build_X_host_resize_s": t_host, "build_X_device_resize_s": t_nat,
                          "frames_per_s_host_resize": nfiles / t_host, "frames_per_s_decode_only": nfiles / t_nat,
                          "pil_resize_ms_per_frame_one_process": t_pil * 1e3}
        print("loading %d PNGs: decode + PIL resize %.2f s (%.0f frames/s), decode only %.2f s (%.0f frames/s); PIL resize "
              "alone %.2f ms per frame in one process" % (nfiles, t_host, nfiles / t_host, t_nat, nfiles / t_nat, t_pil * 1e3),
              flush=True)
        model = M.Model((331, 331, 1), Y0size=576, seed=8)
        wall_s = {}
        for flag in (False, True):
            log = os.path.join(tmp, "log_%d" % flag) + "/"
            t0 = time.time()
            predict_spnet.predict_network(datapath=path, log_dir=log, batch_size=128, model=model, device_resize=flag,
                                          u8_frames=True)
            wall_s[flag] = time.time() - t0
        y_a = model.predict(X_host, batch_size=128)
        y_b = model.predict(X_nat, batch_size=128, resize=True)
        t_pa = wall(lambda: model.predict(X_host, batch_size=128))
        t_pb = wall(lambda: model.predict(X_nat, batch_size=128, resize=True))
        res["predict"] = {"predict_network_host_resize_s": wall_s[False], "predict_network_device_resize_s": wall_s[True],
                          "model_predict_u8_331": t_pa, "model_predict_native_resize": t_pb,
                          "identical_predictions": bool(np.array_equal(y_a, y_b)),
                          "note": "predict_network includes loading the PNGs and drawing one overlay PNG per frame"}
        print("predict_network (%d files, load + predict + overlays): host resize %.2f s, device resize %.2f s; "
              "Model.predict alone (median of 5): 331x331 uint8 frames %.3f s (%.3f-%.3f), native frames + device resize %.3f s "
              "(%.3f-%.3f); identical: %s"
              % (nfiles, wall_s[False], wall_s[True], t_pa["s"], t_pa["min_s"], t_pa["max_s"], t_pb["s"], t_pb["min_s"],
                 t_pb["max_s"], res["predict"]["identical_predictions"]), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=2048)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-files", action="store_true")
    ap.add_argument("--knockouts", action="store_true", help="also time the kernel under the diagnostic knock-out builds")
    args = ap.parse_args()
    res = {}
    kernel_part(res)
    if args.knockouts:
        knockout_part(res)
    if not args.skip_files:
        files_part(res, args.files)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
