#!/usr/bin/env python3
"""Dev tool (GPU box): what the note envelopes of a batch of strike recordings cost on the host and on the device.

`--strikes` recordings (default 64) of `--frames` frames (default 4,096) at 48 kHz and 200 frames a second -- 983,040
samples each -- through a Hann window of 2048 samples, for K = 7 notes (one strike's antinodes) and K = 64 (the kernel's
limit).  The sound is fake_espi.strike_audio_host's: `--distinct` sequences (default 2) are synthesised and repeated to fill
the batch (the kernel has no data-dependent path: its time does not depend on the samples).  Two ways:
  host     audio.note_envelopes_host on the FIRST `--host_strikes` recordings only (default 1; the numpy rule is slow)
  device   audio.note_envelopes_device on ALL recordings, pcm in HBM, results left there
One warm-up round, then `--repeats` rounds in which the two alternate in this one process; median / min / max recordings per
second each.  The device's sums of the first host_strikes recordings are checked against the host's.  Also the kernel alone
(events around back-to-back launches over rotating output buffers).  No threshold: the figures are recorded, not judged.

usage: audio_time.py [--strikes 64] [--frames 4096] [--host_strikes 1] [--distinct 2] [--repeats 5]
                     [--out profiles/audio_time.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.resize_time import gpu_time

RATE, FPS, WINDOW = 48000, 200, 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strikes", type=int, default=64)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--host_strikes", type=int, default=1)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="profiles/audio_time.json")
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "audio_time.py measures on the GPU"
    from spnet_amd import _lib as L
    from spnet_amd import audio as AU
    from spnet_amd import fake_espi as F

    S, T, sh = args.strikes, args.frames, min(args.host_strikes, args.strikes)
    nd = max(1, min(args.distinct, S))
    _, nodes0, nnode0 = (a.cpu().numpy() for a in F.draw_params_device(nd, seed=1))
    distinct, info = F.strike_audio_host(nodes0, nnode0, T, seed=1, rate=RATE, fps=FPS)
    pcm_h = np.ascontiguousarray(distinct[np.arange(S) % nd])
    pcm_d = torch.from_numpy(pcm_h).cuda()
    win, hop = AU.window_table(WINDOW), AU.hop_fraction(RATE, FPS)
    freqs = 440.0 * 2.0 ** ((np.arange(64) * 0.5 + 55 - 69) / 12.0)        # 64 notes a quarter tone apart from G3 up
    res = {"device": torch.cuda.get_device_name(0), "strikes": S, "distinct_strikes": nd, "frames": T, "rate": RATE, "fps": FPS,
           "window": WINDOW, "samples_per_strike": int(pcm_h.shape[1]), "host_strikes": sh,
           "cpus_usable": len(os.sched_getaffinity(0)),
           "note": "the host way runs on the first host_strikes recordings only; its rate is recordings of that run per second"}

    for K in (7, 64):
        steps = AU.note_steps(freqs[:K], RATE)
        got = {}

        def host():
            got["host"] = AU.note_envelopes_host(pcm_h[:sh], None, T, hop, 0, steps, win)

        def device():
            got["device"] = AU.note_envelopes_device(pcm_d, None, T, hop, 0, steps, win)

        ways = (("host", host, sh), ("device", device, S))
        times = {k: [] for k, _, _ in ways}
        for rnd in range(args.repeats + 1):              # round 0 warms up: code objects, allocator
            for name, fn, _ in ways:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(time.perf_counter() - t0)
            if rnd == 0:
                for c in (0, 1):                         # re, im: the same integers
                    assert np.array_equal(got["device"][c][:sh].cpu().numpy(), got["host"][c]), c
        r = {}
        for name, _, n in ways:
            t = sorted(times[name])
            r[name] = {"strikes_per_s": n / t[len(t) // 2], "min_strikes_per_s": n / t[-1], "max_strikes_per_s": n / t[0],
                       "ms_per_strike": 1e3 * t[len(t) // 2] / n, "rounds": len(t), "strikes": n}
            print("K", K, name, json.dumps(r[name]), flush=True)
        r["device_over_host"] = r["device"]["strikes_per_s"] / r["host"]["strikes_per_s"]

        # the kernel alone, on the whole batch
        nrot = 3
        st = L.current_stream()
        dev = [torch.from_numpy(np.array(a)).cuda() for a in (win, steps.view(np.int32), AU.cos_table())]
        lens = torch.full((S,), pcm_h.shape[1], dtype=torch.int32, device="cuda")
        outs = [[torch.empty((S, T, K), dtype=torch.int64, device="cuda") for _ in range(2)] for _ in range(nrot)]
        k = gpu_time(lambda i: L.spnet_note_envelopes(pcm_d.data_ptr(), lens.data_ptr(), S, pcm_h.shape[1], T, 0, hop[0], hop[1],
                                                      dev[0].data_ptr(), WINDOW, dev[1].data_ptr(), K, dev[2].data_ptr(),
                                                      outs[i][0].data_ptr(), outs[i][1].data_ptr(), st), nrot, window_ms=100.0)
        k["us_per_strike"] = k["us"] / S
        k["terms_per_s"] = 2.0 * S * T * K * WINDOW / (k["us"] * 1e-6)    # multiply-adds (re and im) a second
        r["spnet_note_envelopes"] = k
        print("K", K, "spnet_note_envelopes", json.dumps(k), flush=True)
        res["K%d" % K] = r
        del outs, got

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
