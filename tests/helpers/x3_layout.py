"""The bf16x3 plane layout of csrc/x3t.h, undone: shared by tests/test_kernels_gpu.py and tests/test_gemm_x3_gpu.py."""
import torch


def x3_untile(planes, R, K):
    """planes in the pieces layout of csrc/x3t.h -> float64 [3][R16][Kp] (R16, Kp: R, K rounded up to 16 / 32): element
    (r, k) of a plane sits at ((r/16)*nk + k/32)*512 + (r%16)*32 + (((k%32)/8 ^ -((r%16)/4)) & 3)*8 + k%8."""
    nk, rg = (K + 31) // 32, (R + 15) // 16
    p = planes.view(torch.bfloat16).reshape(3, rg, nk, 16, 4, 8).float().cpu().double()
    r16 = torch.arange(16)
    cpos = torch.arange(4)[None, :] ^ ((-(r16 // 4)) & 3)[:, None]            # [r16][chunk] -> stored position
    q = p[:, :, :, r16[:, None], cpos, :]                                     # [3][rg][nk][16][chunk][8]
    return q.permute(0, 1, 3, 2, 4, 5).reshape(3, rg * 16, nk * 32)
