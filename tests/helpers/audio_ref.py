"""The note-envelope rule (include/spnet_hip.h "Note envelopes") restated with Python integers and plain loops: no numpy
arithmetic takes part in the sums.  Tables and arrays come in as anything indexable; every value is passed through int()."""
import numpy as np

M32 = 0xFFFFFFFF


def note_envelopes(pcm, lens, T, hop, offset, steps, window, ctab):
    """(re, im) as int64 arrays [S, T, K] (filled from Python integers).  pcm [S][L]; lens [S] or None; hop = (num, den)."""
    S, L = len(pcm), len(pcm[0]) if len(pcm) else 0
    num, den = int(hop[0]), int(hop[1])
    win = [int(v) for v in window]
    tab = [int(v) for v in ctab]
    st = [int(v) for v in steps]
    re = np.zeros((S, T, len(st)), np.int64)
    im = np.zeros((S, T, len(st)), np.int64)
    for s in range(S):
        n_valid = L if lens is None else min(max(int(lens[s]), 0), L)
        row = [int(v) for v in pcm[s]]
        for t in range(T):
            start = int(offset) + (t * num) // den
            for k, step in enumerate(st):
                r = m = 0
                for i, w in enumerate(win):
                    n = start + i
                    x = row[n] if 0 <= n < n_valid else 0
                    if x == 0:
                        continue                                      # a zero term
                    q = ((i * step) & M32) >> 20
                    r += x * w * tab[q]
                    m += x * w * tab[(q + 3072) & 4095]
                assert -2 ** 63 <= r < 2 ** 63 and -2 ** 63 <= m < 2 ** 63
                re[s, t, k], im[s, t, k] = r, m
    return re, im
