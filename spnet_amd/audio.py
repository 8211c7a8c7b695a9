"""The audio half of the reference's one physics result -- "sympathetic vibrations appear to ramp up in the video well
before you can hear them in the audio recordings (of the same strikes)": how loud each pan note is in a strike's sound
recording at the instant of every video frame (csrc/audio.hip), an onset per note by the same rule as the onset of a
track's ring-count curve, and the lag between the two per track.

THE RULE (include/spnet_hip.h "Note envelopes" states it for the kernel).  pcm int16 [S, L] with len [S]
valid samples a row; frame t = 0 .. T-1 has a window of Wn samples that starts at offset + floor(t hop), hop = rate / fps
samples per frame as an exact rational; note k has the phase step round(f_k / rate 2^32).  For i = 0 .. Wn-1, n = start +
i:  x = pcm[s, n] inside 0 .. len-1, else 0;  q = (uint32)(i step_k) >> 20;  re += x win[i] ctab[q];  im += x win[i]
ctab[(q + 3072) & 4095].  int64 sums of integers: the device and the host give the same arrays, for any split of S or T.
The two tables -- cos_table, window_table -- are built here ONCE and handed to both paths and to the oracle.  The one
floating-point step, envelope(), is shared by both paths.

NOT HANDLED: more than one channel (read_wav keeps the first); anything but PCM16; resampling; pitch detection -- the note
frequencies are given (notes.csv); notes less than two bins (2 rate / Wn Hz) apart leak into each other through the Hann
window; an onset is resolved no finer than the window (2048 samples at 48 kHz: 43 ms, 8.5 frames at 200 frames a second).

  cos_table, window_table, note_steps, hop_fraction   the tables and the integer parameters
  note_envelopes_device    pcm -> (re, im) int64 device tensors [S, T, K]
  note_envelopes_host      the same in numpy int64 (exact; slow)
  envelope                 (re, im) -> amplitude in PCM units, float64 [S, T, K]: one function for both paths
  read_wav / write_wav     PCM16 WAV files (stdlib wave)
  read_notes / write_notes notes.csv: name, freq_hz, cx, cy -- the note's position on the pan in frame pixels
  onset_frame              first index at which a curve reaches frac of its maximum: ONE function for sound and rings
  track_centres, assign_notes, audio_lag, write_lag, write_envelopes     tracks joined to notes, and the lag records

Nothing here imports torch or the HIP library until a device function is called.
"""
import csv
import wave
from fractions import Fraction

import numpy as np

from . import masks as MK

TAB, TAB_SHIFT, TAB_ONE = 4096, 20, 16384                  # csrc/audio_core.h
MAX_K, MIN_WN, MAX_WN, MAX_T, MAX_I32, MAX_OFFSET = 64, 64, 8192, 1 << 20, (1 << 31) - 1, 1 << 40
DEFAULT_WINDOW, DEFAULT_ONSET_FRAC, DEFAULT_NOTE_RADIUS = 2048, 0.1, 40          # choices, not measurements
NOTE_FIELDS = ("name", "freq_hz", "cx", "cy")
LAG_FIELDS = ("note", "freq_hz", "track", "video_onset", "audio_onset", "lag_frames", "lag_ms", "peak_env", "max_rings")

_host = MK.host_array
_TABLES = {}


# ----------------------------------------------------------------------------- tables and integer parameters
def cos_table():
    """int16 [4096]: round(16384 cos(2 pi i / 4096)).  position q + 3072 is the sine of position q."""
    if "cos" not in _TABLES:
        t = np.rint(TAB_ONE * np.cos(2.0 * np.pi * np.arange(TAB, dtype=np.float64) / TAB)).astype(np.int16)
        t.setflags(write=False)
        _TABLES["cos"] = t
    return _TABLES["cos"]


def window_table(Wn=DEFAULT_WINDOW):
    """int16 [Wn]: the Hann window round(32767 * 0.5 * (1 - cos(2 pi i / Wn))), 0 .. 32767.  Entries i <= Wn / 2 are
    computed and entry Wn - i is entry i: the quarter points are ties (16383.5) that a computed cosine breaks either
    way, and the table is symmetric by construction, not by luck."""
    Wn = int(Wn)
    if not MIN_WN <= Wn <= MAX_WN:
        raise ValueError("audio: a window has %d .. %d samples, got %d" % (MIN_WN, MAX_WN, Wn))
    i = np.arange(Wn, dtype=np.int64)
    i = np.minimum(i, Wn - i)
    return np.rint(32767.0 * 0.5 * (1.0 - np.cos(2.0 * np.pi * i.astype(np.float64) / Wn))).astype(np.int16)


def note_steps(freqs, rate):
    """uint32 [K]: the phase step round(f / rate * 2^32) of every note; 0 <= f < rate."""
    f = np.atleast_1d(np.asarray(freqs, np.float64))
    if not (float(rate) > 0 and np.all(np.isfinite(f)) and np.all(f >= 0) and np.all(f < float(rate))):
        raise ValueError("audio: note frequencies are finite, not negative and below the sample rate %r" % (rate,))
    return (np.rint(f / float(rate) * 4294967296.0).astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def hop_fraction(rate, fps):
    """(hop_num, hop_den): rate / fps samples per frame as an exact rational, fps through
    Fraction(fps).limit_denominator(10**6)."""
    F = fps if isinstance(fps, Fraction) else Fraction(fps).limit_denominator(10 ** 6)
    if F <= 0 or Fraction(rate) <= 0:
        raise ValueError("audio: the sample rate and the frame rate are positive, got %r and %r" % (rate, fps))
    hop = Fraction(rate) / F
    return hop.numerator, hop.denominator


def _hop(hop):
    if isinstance(hop, (tuple, list)):
        num, den = int(hop[0]), int(hop[1])
    else:
        h = Fraction(hop)
        num, den = h.numerator, h.denominator
    return num, den


def _args(pcm_shape, T, hop, offset, steps, window, ctab):
    """The checked integer arguments (S, L, T, num, den, offset, steps uint32 [K], window int16 [Wn], ctab int16 [4096])."""
    if len(pcm_shape) != 2:
        raise ValueError("audio: pcm is int16 [S, L], got shape %s" % (tuple(pcm_shape),))
    S, L, T, offset = int(pcm_shape[0]), int(pcm_shape[1]), int(T), int(offset)
    num, den = _hop(hop)
    steps = np.ascontiguousarray(np.atleast_1d(np.asarray(steps)).astype(np.uint32))
    window = np.ascontiguousarray(np.asarray(window).astype(np.int16))
    ctab = cos_table() if ctab is None else np.ascontiguousarray(np.asarray(ctab).astype(np.int16))
    K, Wn = int(steps.size), int(window.size)
    if not (steps.ndim == 1 and window.ndim == 1 and ctab.shape == (TAB,) and 1 <= T <= MAX_T and 1 <= K <= MAX_K
            and MIN_WN <= Wn <= MAX_WN and 1 <= L <= MAX_I32 and 1 <= num <= MAX_I32 and 1 <= den <= MAX_I32
            and abs(offset) <= MAX_OFFSET and S * T * K <= MAX_I32):
        raise ValueError("audio: T 1 .. 2^20, K 1 .. %d notes, a window of %d .. %d samples, L 1 .. 2^31 - 1, hop a ratio of "
                         "integers 1 .. 2^31 - 1, |offset| <= 2^40, S T K <= 2^31 - 1 and a cosine table of %d; got S %d, L %d, "
                         "T %d, K %d, Wn %d, hop %d/%d, offset %d" % (MAX_K, MIN_WN, MAX_WN, TAB, S, L, T, K, Wn, num, den, offset))
    return S, L, T, num, den, offset, steps, window, ctab


def _lens(length, S, L):
    if length is None:
        return np.full(S, L, np.int64)
    length = np.asarray(_host(length)).astype(np.int64).reshape(-1)
    if length.size != S:
        raise ValueError("audio: len has one entry per recording (%d), got %d" % (S, length.size))
    return np.clip(length, 0, L)


# ----------------------------------------------------------------------------- the rule on the host
def note_envelopes_host(pcm, length, T, hop, offset, steps, window, ctab=None, chunk=256):
    """The rule in numpy int64, bit for bit what the kernel gives: (re, im) int64 [S, T, K].  pcm int16 [S, L]; length [S]
    or None (every sample counts); hop a Fraction, an integer or (num, den); window and ctab the tables.  chunk frames of
    [chunk, Wn] int64 at a time (the result does not depend on it)."""
    pcm = np.asarray(_host(pcm))
    if pcm.dtype != np.int16:
        raise TypeError("audio: pcm is int16, got %s" % pcm.dtype)
    S, L, T, num, den, offset, steps, window, ctab = _args(pcm.shape, T, hop, offset, steps, window, ctab)
    lens = _lens(length, S, L)
    K, Wn = steps.size, window.size
    i = np.arange(Wn, dtype=np.uint64)
    q = (((i[:, None] * steps.astype(np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)) >> np.uint64(TAB_SHIFT)).astype(np.int64)
    C, Sn = ctab.astype(np.int64)[q], ctab.astype(np.int64)[(q + 3072) & (TAB - 1)]                  # [Wn, K]
    starts = offset + (np.arange(T, dtype=np.int64) * num) // den
    win = window.astype(np.int64)
    re, im = np.zeros((S, T, K), np.int64), np.zeros((S, T, K), np.int64)
    for s in range(S):
        if lens[s] == 0:
            continue
        row = pcm[s, :lens[s]].astype(np.int64)
        for t0 in range(0, T, int(chunk)):
            idx = starts[t0:t0 + chunk, None] + np.arange(Wn, dtype=np.int64)[None, :]
            inside = (idx >= 0) & (idx < lens[s])
            if not inside.any():
                continue
            xw = np.where(inside, row[np.clip(idx, 0, lens[s] - 1)], 0) * win[None, :]
            re[s, t0:t0 + chunk], im[s, t0:t0 + chunk] = xw @ C, xw @ Sn
    return re, im


# ----------------------------------------------------------------------------- the device side
def note_envelopes_device(pcm, length, T, hop, offset, steps, window, ctab=None, device=None):
    """(re, im) int64 device tensors [S, T, K] on the current stream (csrc/audio.hip): one launch per 65,535 recordings.
    pcm: an int16 device tensor [S, L], or a host array, which is uploaded once; length: int32 device tensor [S], a host
    array, or None (every sample counts).  Only the caller reads anything back."""
    import torch
    from . import _lib as L_
    if isinstance(pcm, torch.Tensor):
        if pcm.dtype != torch.int16 or not pcm.is_cuda:
            raise TypeError("audio: note_envelopes_device takes an int16 device tensor [S, L] or a host array")
        pcm = pcm.contiguous()
        dev = pcm.device
    else:
        pcm = np.ascontiguousarray(pcm)
        if pcm.dtype != np.int16:
            raise TypeError("audio: pcm is int16, got %s" % pcm.dtype)
        dev = torch.device("cuda:0" if device is None else device)
    S, L, T, num, den, offset, steps, window, ctab = _args(tuple(pcm.shape), T, hop, offset, steps, window, ctab)
    K = steps.size
    re, im = (torch.empty((S, T, K), dtype=torch.int64, device=dev) for _ in range(2))
    if S == 0:
        return re, im
    def up(a, kind):                 # (torch wants a writable array)
        a = np.ascontiguousarray(a).view(kind)
        return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)

    if not isinstance(pcm, torch.Tensor):
        pcm = up(pcm, np.int16)
    if isinstance(length, torch.Tensor) and length.is_cuda:
        if length.dtype != torch.int32 or length.numel() != S:
            raise TypeError("audio: a device len is int32 [S]")
        lens = length.contiguous()
    else:
        lens = up(_lens(length, S, L).astype(np.int32), np.int32)
    win_d, step_d, ctab_d = up(window, np.int16), up(steps, np.int32), up(ctab, np.int16)
    with torch.cuda.device(dev):
        L_.spnet_note_envelopes(pcm.data_ptr(), lens.data_ptr(), S, L, T, offset, num, den, win_d.data_ptr(), window.size,
                                step_d.data_ptr(), K, ctab_d.data_ptr(), re.data_ptr(), im.data_ptr(), L_.current_stream())
    return re, im


def envelope(re, im, window):
    """The amplitude in PCM units, float64 of re's shape: sqrt(re^2 + im^2) / (16384 * sum(window)) -- a sine of amplitude A
    at a note's frequency gives A / 2.  The ONE floating-point step, shared by the device and the host path, so their
    envelopes agree bit for bit."""
    r, m = _host(re).astype(np.float64), _host(im).astype(np.float64)
    return np.sqrt(r * r + m * m) / (float(TAB_ONE) * float(np.asarray(window).astype(np.int64).sum()))


def note_curves(pcm, rate, notes, T, fps, offset=0, window=DEFAULT_WINDOW, host=False, device=None):
    """float64 [T, K]: the envelope of every note of notes [(name, freq_hz, cx, cy)] in ONE recording pcm int16 [n] at the
    instants of T frames at fps frames a second, through a Hann window of `window` samples.  On the GPU (the recording goes
    up once per 64 notes, [T, K] integers come back) unless host=True, which runs the numpy rule: the same bits."""
    pcm = np.ascontiguousarray(np.asarray(pcm))
    if pcm.ndim != 1 or pcm.dtype != np.int16 or pcm.size < 1:
        raise ValueError("audio: one recording is a non-empty int16 array [n], got %s %s" % (pcm.dtype, pcm.shape))
    win, hop = window_table(window), hop_fraction(rate, fps)
    steps = note_steps([n[1] for n in notes], rate) if len(notes) else np.zeros(0, np.uint32)
    out = np.zeros((int(T), len(notes)), np.float64)
    run = note_envelopes_host if host else (lambda *a: note_envelopes_device(*a, device=device))
    for k0 in range(0, len(notes), MAX_K):
        re, im = run(pcm[None, :], None, T, hop, offset, steps[k0:k0 + MAX_K], win)
        out[:, k0:k0 + MAX_K] = envelope(re, im, win)[0]
    return out


# ----------------------------------------------------------------------------- files
def read_wav(path):
    """(pcm int16 [n], rate) of a PCM16 WAV file.  A file of several channels is reduced to its FIRST channel; any other
    sample width raises ValueError."""
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2 or w.getcomptype() != "NONE":
            raise ValueError("read_wav: %s has %d-byte samples (%s); only PCM16 is read" % (path, w.getsampwidth(), w.getcomptype()))
        ch, rate = w.getnchannels(), w.getframerate()
        data = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    return np.ascontiguousarray(data.reshape(-1, ch)[:, 0]).astype(np.int16), int(rate)


def write_wav(path, pcm, rate):
    """One channel of PCM16 at `rate` samples a second; pcm is an int16 array [n] (anything else raises ValueError)."""
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16 or pcm.ndim != 1:
        raise ValueError("write_wav: pcm is int16 [n], got %s %s" % (pcm.dtype, pcm.shape))
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(rate))
        w.writeframes(pcm.astype("<i2").tobytes())


def read_notes(path):
    """[(name, freq_hz, cx, cy), ...] of a notes.csv (header NOTE_FIELDS)."""
    with open(path, newline="") as f:
        lines = list(csv.reader(f))
    if not lines or tuple(c.strip() for c in lines[0]) != NOTE_FIELDS:
        raise ValueError("read_notes: %s does not start with the header %s" % (path, ",".join(NOTE_FIELDS)))
    out = []
    for v in lines[1:]:
        if not v:
            continue
        if len(v) != len(NOTE_FIELDS):
            raise ValueError("read_notes: %s: %d fields in %r" % (path, len(v), v))
        out.append((v[0], float(v[1]), float(v[2]), float(v[3])))
    return out


def write_notes(path, notes):
    """notes.csv from [(name, freq_hz, cx, cy), ...]; floats by repr, so they read back exactly."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(NOTE_FIELDS)
        for name, freq, cx, cy in notes:
            w.writerow([str(name), repr(float(freq)), repr(float(cx)), repr(float(cy))])


# ----------------------------------------------------------------------------- onsets, notes and lag
def onset_frame(curve, frac=DEFAULT_ONSET_FRAC):
    """The first index at which curve >= frac * max(curve); -1 for an empty curve or one that is nowhere above 0.  The
    envelope of a note and the ring-count curve of a track both go through this one function."""
    c = np.asarray(curve, np.float64).reshape(-1)
    if c.size == 0 or not c.max() > 0:
        return -1
    return int(np.argmax(c >= float(frac) * c.max()))


def track_curves(table, T):
    """{track: float64 [T]} -- the ring count of every track of a track table (tracks.track_table records) on the movie's
    frame grid, 0 where the track has no detection; frames outside 0 .. T-1 are left out."""
    out = {}
    for rec in table:
        if 0 <= rec[0] < T:
            out.setdefault(rec[2], np.zeros(T, np.float64))[rec[0]] = rec[9]
    return out


def track_centres(table):
    """[(track, n, mean cx, mean cy), ...] in track order: a track table's summary rows with the mean centre."""
    acc = {}
    for rec in table:
        a = acc.setdefault(rec[2], [0, 0.0, 0.0])
        a[0], a[1], a[2] = a[0] + 1, a[1] + rec[4], a[2] + rec[5]
    return [(tr, a[0], a[1] / a[0], a[2] / a[0]) for tr, a in sorted(acc.items())]


def assign_notes(centres, notes, radius=DEFAULT_NOTE_RADIUS):
    """[track or None per note]: every track of centres [(track, n, cx, cy)] goes to its nearest note centre if that is
    within `radius` pixels (the lower note index on equal distance) and to no note beyond it; a note that several tracks
    claim keeps the longest (largest n), the lower track id on a tie."""
    best = [None] * len(notes)
    for tr, n, cx, cy in centres:
        d2 = [(cx - nx) ** 2 + (cy - ny) ** 2 for _, _, nx, ny in notes]
        if not d2:
            continue
        k = int(np.argmin(d2))
        if d2[k] > float(radius) ** 2:
            continue
        if best[k] is None or (n, -tr) > (best[k][1], -best[k][0]):
            best[k] = (tr, n)
    return [None if b is None else b[0] for b in best]


def audio_lag(table, notes, env, fps, frac=DEFAULT_ONSET_FRAC, radius=DEFAULT_NOTE_RADIUS):
    """One record per note in LAG_FIELDS: (note, freq_hz, track, video_onset, audio_onset, lag_frames, lag_ms, peak_env,
    max_rings).  table: tracks.track_table records (or a truth table); env float64 [T, K], column k the envelope of note
    k.  audio_onset = onset_frame(env[:, k]); a note's track is assign_notes'; video_onset = onset_frame of that track's
    ring curve on the same T frames; lag = audio - video, in frames and in milliseconds at fps.  track, video_onset,
    max_rings and the lag fields are None without a track, the lag fields also where either onset is -1."""
    env = np.asarray(env, np.float64)
    if env.ndim != 2 or env.shape[1] != len(notes):
        raise ValueError("audio_lag: env is [T, %d notes], got %s" % (len(notes), env.shape))
    T = env.shape[0]
    owner = assign_notes(track_centres(table), notes, radius)
    curves = track_curves(table, T)
    out = []
    for k, (name, freq, _, _) in enumerate(notes):
        a_on = onset_frame(env[:, k], frac)
        peak = float(env[:, k].max()) if T else 0.0
        tr = owner[k]
        if tr is None or tr not in curves:
            out.append((name, float(freq), None, None, a_on, None, None, peak, None))
            continue
        v_on = onset_frame(curves[tr], frac)
        lag = a_on - v_on if a_on >= 0 and v_on >= 0 else None
        out.append((name, float(freq), int(tr), v_on, a_on, lag, None if lag is None else 1000.0 * lag / float(fps), peak,
                    float(curves[tr].max())))
    return out


def _suffixed(path, suffix):
    from .tracks import _suffixed as sfx
    return sfx(path, suffix)


def lag_path(path):
    return _suffixed(path, "_lag")


def envelopes_path(path):
    return _suffixed(path, "_envelopes")


def write_lag(path, records):
    """The lag records as CSV (header LAG_FIELDS; None as an empty field, floats by repr)."""
    from .tracks import _write_csv
    _write_csv(path, LAG_FIELDS, records)


def write_envelopes(path, env, notes):
    """One row per frame, one column per note (header: frame, then the note names); floats by repr."""
    from .tracks import _write_csv
    env = np.asarray(env, np.float64)
    _write_csv(path, ("frame",) + tuple(str(n[0]) for n in notes), [(t,) + tuple(float(v) for v in row) for t, row in enumerate(env)])
