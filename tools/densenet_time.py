"""DenseNet121 timing on one MI355X: training images/s (384x512, batch 32), inference frames/s (batch 128), the per-family
kernel table of one training step (KernelTimer), and an A/B of the BN+ReLU-on-load 1x1 GEMM against the materialising
path on one layer of each dense block, forward and data gradient (ab_layers).

    python tools/densenet_time.py [--train-batch 32] [--infer-batch 128] [--steps 5]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def ab_layers(n=20):
    """On the last layer of each block at 384x512, batch 32 (c = Cb - 32, N = 128):
    forward   spnet_gemm_f32_bnrelu (library tile and the tiles in TILES) against the materialising path
              spnet_dense_apply_ld + spnet_gemm_f32.  spnet_dense_apply_ld is spnet_bn_apply's arithmetic
              (act(fmaf(x, scale, shift))) with a row stride: spnet_bn_apply itself needs a contiguous [M][c] input, so the
              issue's spnet_bn_apply + spnet_gemm_f32 baseline would pay one more copy of x[:, :c].
    data gradient  the engine's path (dgrad GEMM -> dz, spnet_dense_consumer_bwd + _fin into G / u / v) against the
              materialising per-consumer path from existing kernels: the same GEMM, x[:, :c] copied out of the concat
              buffer (spnet_copy_cols), spnet_bn_bwd (ReLU) -> dx, dx added onto G (spnet_copy_cols, accumulate)."""
    from spnet_amd import _lib as L
    from spnet_amd.densenet import densenet_blocks
    st = L.current_stream()
    rows = []
    h, w = 48, 64
    for name, c0, nl, trans in densenet_blocks():
        B = 32
        M = B * h * w
        Cb = c0 + 32 * nl
        c = Cb - 32
        cld = (c + 31) // 32 * 32
        x = torch.randn(M, Cb, device="cuda")
        coef = torch.zeros(3 * cld, device="cuda")
        coef[:c] = 1.0
        coef[2 * cld:2 * cld + c] = 0.1
        Wt = torch.randn(c, 128, device="cuda")
        y = torch.empty(M, 128, device="cuda")
        z = torch.empty(M, c, device="cuda")
        ws = torch.empty(16 << 20, device="cuda")

        def fused(tile):
            return lambda: L.spnet_gemm_f32_bnrelu(x.data_ptr(), Cb, coef.data_ptr(), cld, Wt.data_ptr(), 128, y.data_ptr(),
                                                   128, M, 128, c, tile, None, None, st)

        def mat():
            L.spnet_dense_apply_ld(x.data_ptr(), Cb, M, c, coef.data_ptr(), cld, 1, z.data_ptr(), c, st)
            L.spnet_gemm_f32(z.data_ptr(), 0, c, Wt.data_ptr(), 1, 128, y.data_ptr(), 128, M, 128, c, 0, ws.data_ptr(),
                             ws.numel(), None, 0, st)
        tiles = {t: _time(fused(t), n) * 1e6 for t in TILES}
        tf, tm = tiles[0], _time(mat, n) * 1e6
        byts = 4.0 * (M * c + c * 128 + M * 128)
        # data gradient
        dy = torch.randn(M, 128, device="cuda")
        dz = torch.empty(M, c, device="cuda")
        G = torch.zeros(M, Cb, device="cuda")
        u, v = torch.zeros(Cb, device="cuda"), torch.zeros(Cb, device="cuda")
        mean, invstd = torch.zeros(Cb, device="cuda"), torch.ones(Cb, device="cuda")
        gamma, beta = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
        dgam, dbet = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
        P = int(L.spnet_dense_rows(M))
        part = torch.empty(P * 2 * c, device="cuda")
        xc, dx = torch.empty(M, c, device="cuda"), torch.empty(M, c, device="cuda")
        small = torch.empty(3 * c, device="cuda")

        def dgemm():
            L.spnet_gemm_f32(dy.data_ptr(), 0, 128, Wt.data_ptr(), 0, 128, dz.data_ptr(), c, M, c, 128, 0, ws.data_ptr(),
                             ws.numel(), None, 0, st)

        def dgrad_engine():
            dgemm()
            L.spnet_dense_consumer_bwd(dz.data_ptr(), c, x.data_ptr(), Cb, M, c, coef.data_ptr(), cld, mean.data_ptr(),
                                       invstd.data_ptr(), gamma.data_ptr(), 1, G.data_ptr(), Cb, part.data_ptr(), st)
            L.spnet_dense_consumer_fin(part.data_ptr(), P, c, gamma.data_ptr(), dgam.data_ptr(), dbet.data_ptr(),
                                       u.data_ptr(), v.data_ptr(), st)

        def dgrad_mat():
            dgemm()
            L.spnet_copy_cols(x.data_ptr(), Cb, xc.data_ptr(), c, M, c, 0, st)
            L.spnet_bn_bwd(xc.data_ptr(), dz.data_ptr(), M, c, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
                           invstd.data_ptr(), 1, dx.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), small.data_ptr(),
                           ws.data_ptr(), st)
            L.spnet_copy_cols(dx.data_ptr(), c, G.data_ptr(), Cb, M, c, 1, st)
        de, dm = _time(dgrad_engine, n) * 1e6, _time(dgrad_mat, n) * 1e6
        rows.append(dict(block=name, M=M, c=c, fwd_fused_us=tf, fwd_fused_by_tile_us=tiles, fwd_materialising_us=tm,
                         fwd_fused_GBps=byts / tf / 1e3, fwd_fused_TFLOPs=2.0 * M * c * 128 / tf / 1e6,
                         dgrad_engine_us=de, dgrad_materialising_us=dm, dgrad_gemm_us=_time(dgemm, n) * 1e6))
        if trans:
            h, w = h // 2, w // 2
    return rows


TILES = (0, 1, 2, 7, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-batch", type=int, default=32)
    ap.add_argument("--infer-batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    from spnet_amd.engine import Engine, KernelTimer
    H, W = 384, 512
    out = {}
    e = Engine(H, W, a.train_batch, backbone="DenseNet121")
    X = torch.rand(a.train_batch, H, W, 1, device="cuda") * 2 - 1
    Y = torch.rand(a.train_batch, 576, device="cuda")
    dt = _time(lambda: e.train_step(X, Y, 1e-5), a.steps)
    out["train_images_per_s"] = a.train_batch / dt
    e.prof = KernelTimer()
    e.train_step(X, Y, 1e-5)
    torch.cuda.synchronize()
    out["kernels_ms"] = {k: round(v[1], 3) for k, v in sorted(e.prof.totals().items())}
    fam = e.prof.totals().get("dense_bnrelu_gemm")
    e.prof = None
    del e
    torch.cuda.empty_cache()
    ei = Engine(H, W, a.infer_batch, backbone="DenseNet121", train=False)
    ei.x_in.copy_(torch.rand(a.infer_batch, H, W, 1, device="cuda") * 2 - 1)
    dt = _time(lambda: ei.predict_step(), a.steps)
    out["infer_frames_per_s"] = a.infer_batch / dt
    if fam:
        out["bnrelu_gemm_launches_ms"] = [fam[0], round(fam[1], 3)]
    del ei
    torch.cuda.empty_cache()
    out["ab_bnrelu_vs_materialising"] = ab_layers()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
