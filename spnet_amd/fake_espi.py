"""Synthetic 'fake-ESPI' frames + labels: the benchmark / test input distribution.

Follows the reference generator gen_fake_espi.py:60-279 up to, but excluding, the band-pass mix-up
with the author's private real images (augmentation.py:10-62): 512x384 grey canvas at 128, wavy dark
bands (draw_waves :60-80), 1..7 non-overlapping ringed ellipses (draw_antinodes :145-206, draw_rings
:101-114), additive clipped N(40,40) noise, 50 % Bernoulli pixel dropout.  Rasterisation uses PIL
(OpenCV is not available); the parameter draws follow the reference's RNG call order (one `random.Random` +
one numpy RandomState per frame: checked against oracle/espi_ref.py, which is pinned to the reference's own
draws), the pixels are statistically, not bitwise, OpenCV's.  Exactly one PNG per CSV is written (the reference also writes
a *_bp.png that would trip build_dataset's file-count assertion, utils.py:455-459).

The band-pass mix-up with real frames (gen_fake_espi.py:266-271) is opt-in: generate_device(bandpass_real=...) returns
the mixed frames, write_dataset(bandpass_real=..., bp_path=...) writes them as a dataset of their own.  Its draws come
from per-frame streams derived from (not equal to) the frame seeds: deterministic in (n, seed), independent of `chunk`.
"""
import os

import numpy as np
from PIL import Image, ImageDraw

IM_W, IM_H = 512, 384
MIN_LINE_WIDTH = 4


def _ellipse_pts(center, axes, angle_deg, n=90):
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    th = np.deg2rad(-angle_deg)            # the reference passes -angle to cv2.ellipse (utils.py:50)
    x, y = axes[0] * np.cos(t), axes[1] * np.sin(t)
    return [(float(center[0] + u * np.cos(th) - v * np.sin(th)), float(center[1] + u * np.sin(th) + v * np.cos(th)))
            for u, v in zip(x, y)]


def _ellipse_box(center, axes, angle):
    rad = np.radians(angle)
    dx = np.sqrt(axes[0] ** 2 * np.cos(rad) ** 2 + axes[1] ** 2 * np.sin(rad) ** 2)
    dy = np.sqrt(axes[0] ** 2 * np.sin(rad) ** 2 + axes[1] ** 2 * np.cos(rad) ** 2)
    return [center[0] - dx, center[1] - dy, center[0] + dx, center[1] + dy]


def _overlaps(a, b):
    return not (a[2] < b[0] or a[0] > b[2] or a[3] < b[1] or a[1] > b[3])


def draw_params(seed, count_range=(1, 7)):
    """All random PARAMETERS of one frame, drawn in the reference generator's own RNG call order -- it interleaves Python's
    `random` module and numpy's generator, and so does this: one random.Random(seed) and one RandomState(seed) per frame
    (the reference seeds both global generators once per run, gen_fake_espi.py:317-318; a generator pair per frame lets
    frames be generated in any order and in parallel).
    waves = (amp, wavelength, thickness, slope, spacing) (draw_waves, gen_fake_espi.py:60-80) and
    nodes = [(cx, cy, a, b, angle, rings, ring_start)] (draw_antinodes :145-206 incl. the non-overlap rejection
    loop, draw_rings' rand_start :107).  Returns (waves, nodes, (rnd, rs)) -- the generators continue with the sensor-model
    draws of the host rasteriser.  count_range = (lo, hi) inclusive: the number of antinodes drawn per frame -- (1, 7) is
    the reference's current generator (gen_fake_espi.py:250-251); its comments there date that to 'Nov 11 2020 increasing
    from 6 to 7 ... elminating 0', i.e. the published Dataset-A run was generated with (0, 6): 3.0 objects per frame."""
    import random
    rnd, rs = random.Random(seed), np.random.RandomState(seed)
    amp = rnd.randint(10, 200)
    wavelength = rnd.randint(100, IM_W // 2)
    thick = rnd.randint(15, 40)
    slope = 3 * (rs.rand() - .5)
    spacing = rnd.randint(thick + thick * int(abs(1.5 * slope)), IM_H // 3)
    waves = (amp, wavelength, thick, slope, spacing)
    boxes, nodes = [], []
    for _ in range(rnd.randint(count_range[0], count_range[1])):
        axes = sorted((rnd.randint(15, int(IM_W / 3.5)), rnd.randint(15, int(IM_H / 3.5))), reverse=True)
        rings = rnd.randint(1, min(axes[1] // 8, 11))
        if axes[1] / rings < MIN_LINE_WIDTH:
            rings = axes[1] // MIN_LINE_WIDTH
        center = (rnd.randint(axes[0], IM_W - axes[0]), rnd.randint(axes[1], IM_H - axes[1]))
        angle = rnd.randint(1, 179)
        box = _ellipse_box(center, axes, angle)
        tries = 0
        while (any(_overlaps(box, b) for b in boxes) or box[0] < 0 or box[2] > IM_W or box[1] < 0 or box[3] > IM_H) \
                and tries < 2000:
            tries += 1
            axes = sorted((rnd.randint(25, IM_W // 3), rnd.randint(25, IM_H // 3)), reverse=True)
            if axes[1] / rings < MIN_LINE_WIDTH:
                rings = axes[1] // MIN_LINE_WIDTH
            center = (rnd.randint(axes[0], IM_W - axes[0]), rnd.randint(axes[1], IM_H - axes[1]))
            angle = rnd.randint(1, 180)
            box = _ellipse_box(center, axes, angle)
        if tries < 2000:
            nodes.append((center[0], center[1], axes[0], axes[1], angle, rings, int(rs.choice([0, 1]))))
            boxes.append(box)
    return waves, nodes, (rnd, rs)


def _draw_waves(d, waves):
    amp, wavelength, thick, slope, spacing = waves
    xs = np.arange(IM_W)
    base = slope * xs + amp * np.cos(xs / wavelength)
    for j in range(60 + IM_H // spacing):
        y0 = j * spacing - IM_W * abs(slope)
        ys = (y0 + base).astype(np.int64)
        if ys.max() < -thick or ys.min() > IM_H + thick:
            continue
        d.line(list(zip(xs.tolist(), ys.tolist())), fill=0, width=thick, joint="curve")


def _draw_rings(d, center, axes, angle, rings, start):
    nwb = max(2 * rings, 1)
    thick = max(int(round(min(axes) / nwb)), 1)
    for j in range(nwb):
        col = 0 if (start + j) % 2 == 0 else 138
        ax = [a * (j + 1) / (nwb + 1) for a in axes]
        pts = _ellipse_pts(center, ax, angle)
        d.line(pts + [pts[0]], fill=col, width=thick, joint="curve")


def raster_host(waves, nodes):
    """The noise-free canvas of one frame, rasterised with PIL: uint8 [384,512]."""
    img = Image.new("L", (IM_W, IM_H), 128)
    d = ImageDraw.Draw(img)
    _draw_waves(d, waves)
    for cx, cy, a, b, angle, rings, start in nodes:
        _draw_rings(d, (cx, cy), (a, b), angle, rings, start)
    return np.asarray(img, dtype=np.uint8)


def gen_frame(seed):
    """One frame: (uint8 [384,512] image, [(cx,cy,a,b,angle,rings), ...])."""
    waves, nodes, (rnd, rs) = draw_params(seed)
    a = raster_host(waves, nodes).astype(np.float32)
    if rs.random_sample() <= 0.3:             # blur_inplace (augmentation.py:66-70): a no-op on the pixels, consumes RNG
        rnd.choice([3, 7])
    noise = np.clip(np.rint(rs.normal(40, 40, a.shape)), 0, 255)      # cv2.randn into a uint8 image saturates
    a = np.minimum(a + noise, 255)
    a *= rs.choice([0, 1], size=a.shape)                                # drop half of the pixels (:262-264)
    return a.astype(np.uint8), [n[:6] for n in nodes]


def frame_seeds(n, seed, first=0):
    return [seed * 1000003 + i for i in range(first, first + n)]


def bandpass_seeds(n, seed, first=0):
    """Seeds of the per-frame band-pass draws: a hash of the frame seed, not the seed itself (the frame's own streams
    stay as they are)."""
    return [((s * 2654435761) ^ 0x5BD1E995) % (2 ** 32) for s in frame_seeds(n, seed, first)]


def _cached_table(cache, make, device):
    """A constant table computed once on the host (make() -> numpy array, in float64 arithmetic) and uploaded once per
    device: the numpy array for device None, else the cached device tensor.  `cache` is the table's own dict."""
    if "host" not in cache:
        cache["host"] = make()
    if device is None:
        return cache["host"]
    import torch
    key = str(torch.device(device))
    if key not in cache:
        cache[key] = torch.from_numpy(cache["host"]).to(device)
    return cache[key]


_TRIG2 = {}


def trig2_table(device=None):
    """(cos^2, sin^2) of the whole degrees 0..180 as float32 [181,2], computed in float64: the table the device sampler's
    box test reads (spnet_fake_espi_params; no sinf / cosf on the device, so a host restatement has the same bits).
    device: a cached device tensor instead of the numpy array."""
    def make():
        rad = np.radians(np.arange(181, dtype=np.float64))
        return np.stack([np.cos(rad) ** 2, np.sin(rad) ** 2], 1).astype(np.float32)
    return _cached_table(_TRIG2, make, device)


def draw_params_device(n, seed=0, device="cuda:0", count_range=(1, 7), first_frame=0, want_tries=False):
    """The parameters of the global frames first_frame .. first_frame + n - 1 drawn by spnet_fake_espi_params (csrc/
    espi_params.hip): (waves [n,5], nodes [n,7,8], nnode [n]) device tensors in the layout spnet_fake_espi reads
    [, tries [n,7] int32: the accepted try per antinode drawn, -1 dropped, -2 not drawn].  Same logic and distributions as
    draw_params, a stream of its own (counter based: a frame's parameters depend on (seed, its global index) only -- not on
    n, nor on how a range of frames is split into calls).  Enqueued on the current stream; nothing is copied to the host."""
    import torch
    from . import _lib as L
    dev = torch.device(device)
    waves = torch.empty((n, 5), dtype=torch.float32, device=dev)
    nodes = torch.empty((n, 7, 8), dtype=torch.float32, device=dev)
    nnode = torch.empty((n,), dtype=torch.int32, device=dev)
    tries = torch.empty((n, 7), dtype=torch.int32, device=dev) if want_tries else None
    with torch.cuda.device(dev):
        L.spnet_fake_espi_params(int(first_frame), n, IM_H, IM_W, int(seed) & 0xFFFFFFFF, int(count_range[0]),
                                 int(count_range[1]), trig2_table(dev).data_ptr(), waves.data_ptr(), nodes.data_ptr(),
                                 nnode.data_ptr(), L.ptr(tries), torch.cuda.current_stream(dev).cuda_stream)
    return (waves, nodes, nnode, tries) if want_tries else (waves, nodes, nnode)


def labels_from_params(nodes, nnode):
    """Label rows [[(cx, cy, a, b, angle, rings), ...], ...] (Python ints, what generate_device returns) of device (or
    host) parameter arrays nodes [n,7,8], nnode [n]; device tensors cross to the host in ONE copy."""
    if hasattr(nodes, "is_cuda"):
        import torch
        n = int(nnode.shape[0])
        packed = torch.cat([nodes.reshape(n, 56), nnode.reshape(n, 1).to(torch.float32)], 1).cpu().numpy()
        nodes, nnode = packed[:, :56].reshape(n, 7, 8), packed[:, 56]
    rows = np.asarray(nodes)[:, :, :6].astype(np.int64).tolist()
    return [[tuple(r) for r in fr[:int(k)]] for fr, k in zip(rows, np.asarray(nnode))]


def rows_from_params(nodes, nnode):
    """Device parameter arrays nodes [n,7,8], nnode [n] -> (rows float64 [n,7,6], count int32 [n]) device tensors in
    augmentation.pad_metadata's layout: the values labels_from_params reads back (whole numbers), left in HBM."""
    return nodes[..., :6].trunc().double().contiguous(), nnode.contiguous()


# ----------------------------------------------------------------------------- strike sequences (csrc/espi_strike.hip)
STRIKE_MAX_T, STRIKE_MAX_J, STRIKE_KEY = 4096, 8, 0x51ed270b


def _check_strike(S, T, jitter, first_sequence):
    if not (S >= 0 and 1 <= T <= STRIKE_MAX_T and 0 <= jitter <= STRIKE_MAX_J and first_sequence >= 0
            and S * T <= 2 ** 31 - 1 and 7 * (first_sequence + S) <= 2 ** 31 - 2):
        raise ValueError("strike: S >= 0, T 1 .. %d, jitter 0 .. %d, first_sequence >= 0, S * T and the identities within "
                         "int32; got S %r, T %r, jitter %r, first_sequence %r" % (STRIKE_MAX_T, STRIKE_MAX_J, S, T, jitter,
                                                                                   first_sequence))


def strike_envelope(t, onset, rise, hold, decay):
    """The envelope 0 .. 256 of the strike rule (include/spnet_hip.h "Strike sequences") on int64 arrays."""
    peak = onset + rise
    after = peak + hold + 1
    e = np.where(t < peak, 256 * (t - onset + 1) // (rise + 1),
                 np.where(t < after, 256, np.maximum(256 - 256 * (t - after + 1) // (decay + 1), 0)))
    return np.where(t < onset, 0, e)


def _strike_draws(nodes0, nnode0, T, seed, first_sequence):
    """The per-slot draws of the strike rule for base rows nodes0 [S,7,8], nnode0 [S]: (g [S], skey [S], nn [S], valid [S,7],
    is_struck [S,7], ek [S,7] = key(0, j), onset, rise, hold, decay, R [S,7]), int64 but for the uint64 keys.  One place
    for the frames (strike_params_host) and the sound (strike_audio_host)."""
    from .augmentation import _keyed_draw, _mix32
    S = int(nodes0.shape[0])
    nn = np.clip(np.asarray(nnode0, np.int64), 0, 7)
    u64 = np.uint64

    g = np.arange(S, dtype=np.int64) + int(first_sequence)
    skey = _mix32(_mix32(_mix32(u64((int(seed) & 0xFFFFFFFF) ^ STRIKE_KEY)) + (g.astype(u64) & u64(0xFFFFFFFF)))
                  ^ (g.astype(u64) >> u64(32)))
    j = np.arange(7, dtype=np.int64)
    valid = (j[None, :] < nn[:, None]) & (nodes0[:, :, 7] != 0)                       # [S,7]
    struck = np.where(valid.any(1), valid.argmax(1), 7)
    ek = _mix32(skey[:, None] + j.astype(u64)[None, :])                               # key(0, j)
    is_struck = j[None, :] == struck[:, None]
    onset = np.where(is_struck, 0, _randint(_keyed_draw(ek, 0), 0, T // 2))
    rise = np.where(is_struck, 0, _randint(_keyed_draw(ek, 1), 1, max(T // 4, 1)))
    hold = _randint(_keyed_draw(ek, 2), 0, T // 4)
    decay = _randint(_keyed_draw(ek, 3), 1, T)
    with np.errstate(invalid="ignore"):
        R = np.where(nodes0[:, :, 5] == nodes0[:, :, 5], np.clip(nodes0[:, :, 5], 0, 255), 0).astype(np.int64)
    return g, skey, nn, valid, is_struck, ek, onset, rise, hold, decay, R


def _randint(u, lo, hi):
    """randint of the counter stream (include/spnet_hip.h) on uint64 arrays holding uint32 draws."""
    return lo + ((u * np.uint64(max(hi - lo + 1, 1))) >> np.uint64(32)).astype(np.int64)


def strike_params_host(waves0, nodes0, nnode0, T, seed=0, jitter=0, first_sequence=0):
    """spnet_fake_espi_strike in numpy, bit for bit: base arrays waves0 [S,5], nodes0 [S,7,8], nnode0 [S] (frame-0
    parameters, row s for the global sequence first_sequence + s) -> (waves float32 [S*T,5], nodes float32 [S*T,7,8], nnode
    int32 [S*T], ident int32 [S*T,7]); frame s * T + t is time step t of sequence s."""
    from .augmentation import _keyed_draw, _mix32
    waves0, nodes0 = np.asarray(waves0, np.float32), np.asarray(nodes0, np.float32)
    S, T, J = int(nodes0.shape[0]), int(T), int(jitter)
    _check_strike(S, T, J, int(first_sequence))
    u64, randint = np.uint64, _randint
    g, skey, nn, valid, _, _, onset, rise, hold, decay, R = _strike_draws(nodes0, nnode0, T, seed, first_sequence)
    j = np.arange(7, dtype=np.int64)
    t = np.arange(T, dtype=np.int64)[None, :, None]
    env = strike_envelope(t, onset[:, None, :], rise[:, None, :], hold[:, None, :], decay[:, None, :])
    rings = np.where(valid[:, None, :], (R[:, None, :] * env + 128) >> 8, 0)         # [S,T,7]
    present = rings >= 1
    jk = _mix32(skey[:, None, None] + (((j + 1) << 12)[None, None, :] | t).astype(u64))
    nodes = np.zeros((S, T, 7, 8), np.float32)
    nodes[..., 0] = nodes0[:, None, :, 0] + randint(_keyed_draw(jk, 0), -J, J).astype(np.float32)
    nodes[..., 1] = nodes0[:, None, :, 1] + randint(_keyed_draw(jk, 1), -J, J).astype(np.float32)
    nodes[..., 2:5] = nodes0[:, None, :, 2:5]
    nodes[..., 5] = rings
    nodes[..., 6] = nodes0[:, None, :, 6]
    nodes[..., 7] = 1
    nodes[~present] = 0
    ident = np.where(present, 1 + 7 * g[:, None, None] + j[None, None, :], 0).astype(np.int32)
    waves = np.repeat(waves0[:, :5], T, axis=0)
    return (np.ascontiguousarray(waves), nodes.reshape(S * T, 7, 8), np.repeat(nn.astype(np.int32), T),
            ident.reshape(S * T, 7))


STRIKE_AUDIO_SHIFT, STRIKE_AUDIO_MAX_LAG, STRIKE_AUDIO_MAX_NOISE, STRIKE_AUDIO_MIN_RATE = 18, 64, 1024, 16000
TRUTH_AUDIO_FIELDS = ("ident", "name", "freq_hz", "video_onset", "audio_onset")
_PITCH_NAMES = ("C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B")


def strike_audio_host(nodes0, nnode0, T, seed=0, first_sequence=0, rate=48000, fps=200, lag=4, noise=8):
    """The SOUND of strike sequences, the addendum of the strike rule (include/spnet_hip.h "Strike sequences"): host numpy,
    integers after the note steps.  Every valid slot is a note whose pitch is drawn (draw 4 of its envelope key), whose
    loudness follows the slot's own ring-count envelope `lag` frames late (the struck slot: at once), so that the truth a
    lag analysis (spnet_amd/audio.py) has to recover is "a sympathetic note is audible `lag` frames after it is visible".
    nodes0 [S,7,8], nnode0 [S]: the base rows strike_params_host evolves; the frames and labels do not depend on anything
    here.  hop = rate / fps samples per frame (audio.hop_fraction).  -> (pcm int16 [S, floor(T hop)], info): info is a
    dict of [S,7] arrays -- valid, struck (bool), pitch (MIDI), freq (Hz, float64), step (uint32), lag, onset, rise, hold,
    decay, R (int64) -- and name, a list of 7 note names per sequence."""
    from . import audio as AU
    from .augmentation import _keyed_draw, _mix32
    nodes0 = np.asarray(nodes0, np.float32)
    S, T, lag, noise = int(nodes0.shape[0]), int(T), int(lag), int(noise)
    _check_strike(S, T, 0, int(first_sequence))
    if not (0 <= lag <= STRIKE_AUDIO_MAX_LAG and 0 <= noise <= STRIKE_AUDIO_MAX_NOISE and rate == int(rate)
            and int(rate) >= STRIKE_AUDIO_MIN_RATE):
        raise ValueError("strike audio: lag 0 .. %d frames, noise 0 .. %d, a whole sample rate of at least %d; got lag %r, "
                         "noise %r, rate %r" % (STRIKE_AUDIO_MAX_LAG, STRIKE_AUDIO_MAX_NOISE, STRIKE_AUDIO_MIN_RATE, lag, noise, rate))
    num, den = AU.hop_fraction(int(rate), fps)
    u64, M32 = np.uint64, np.uint64(0xFFFFFFFF)
    _, _, _, valid, is_struck, ek, onset, rise, hold, decay, R = _strike_draws(nodes0, nnode0, T, seed, first_sequence)
    pitch = 60 + 5 * np.arange(7, dtype=np.int64)[None, :] + _randint(_keyed_draw(ek, 4), 0, 2)
    freq = 440.0 * 2.0 ** ((pitch - 69).astype(np.float64) / 12.0)
    step = AU.note_steps(freq.reshape(-1), int(rate)).reshape(S, 7)
    lag_j = np.where(is_struck, 0, lag).astype(np.int64)
    Ls = (T * num) // den
    n = np.arange(Ls, dtype=np.int64)
    frame = (n * den) // num
    ctab = AU.cos_table().astype(np.int64)
    pcm = np.zeros((S, Ls), np.int16)
    for s in range(S):
        acc = np.zeros(Ls, np.int64)
        for j in np.flatnonzero(valid[s]):
            e = strike_envelope(frame - lag_j[s, j], onset[s, j], rise[s, j], hold[s, j], decay[s, j])
            q = ((n.astype(u64) * u64(step[s, j])) & M32) >> u64(AU.TAB_SHIFT)
            acc += R[s, j] * e * ctab[(q.astype(np.int64) + 3072) & (AU.TAB - 1)]
        nkey = _keyed_draw(ek[s, 0], 5)
        draw = _mix32(nkey ^ ((n.astype(u64) & M32) * u64(0x85ebca6b) + u64(0xc2b2ae35) & M32))     # u(nkey, low32(n))
        pcm[s] = np.clip((acc >> STRIKE_AUDIO_SHIFT) + _randint(draw, -noise, noise), -32768, 32767)
    names = [["%s%d" % (_PITCH_NAMES[p % 12], p // 12 - 1) for p in row] for row in pitch.tolist()]
    info = {"valid": valid, "struck": is_struck & valid, "pitch": pitch, "freq": freq, "step": step, "lag": lag_j, "onset": onset,
            "rise": rise, "hold": hold, "decay": decay, "R": R, "name": names}
    return pcm, info


def strike_audio_truth(info, s, T, first_sequence=0, frac=None):
    """What a lag analysis of sequence s (row s of info, the global sequence first_sequence + s) should find: one record
    (ident, name, freq_hz, video_onset, audio_onset) per valid slot whose ring count ever reaches 1.  video_onset =
    audio.onset_frame of the truth ring curve (R e(t) + 128) >> 8, audio_onset = onset_frame of the loudness the sound was
    synthesised with, R e(t - lag), both on the frame grid, at frac (default audio.DEFAULT_ONSET_FRAC)."""
    from . import audio as AU
    frac = AU.DEFAULT_ONSET_FRAC if frac is None else frac
    t = np.arange(int(T), dtype=np.int64)
    out = []
    for j in np.flatnonzero(info["valid"][s]):
        args = tuple(info[k][s, j] for k in ("onset", "rise", "hold", "decay"))
        rings = (info["R"][s, j] * strike_envelope(t, *args) + 128) >> 8
        if not (rings >= 1).any():
            continue
        loud = info["R"][s, j] * strike_envelope(t - info["lag"][s, j], *args)
        out.append((1 + 7 * (int(first_sequence) + s) + int(j), info["name"][s][j], float(info["freq"][s, j]),
                    AU.onset_frame(rings, frac), AU.onset_frame(loud, frac)))
    return out


def strike_params_device(S, T, seed=0, jitter=0, first_sequence=0, count_range=(1, 7), device="cuda:0"):
    """The parameters of S strike sequences of T frames (csrc/espi_strike.hip): the frame-0 parameters of the global frames
    first_sequence .. first_sequence + S - 1 from draw_params_device, evolved on the device.  -> (waves [S*T,5], nodes
    [S*T,7,8], nnode [S*T], ident int32 [S*T,7]) device tensors; enqueued on the current stream, nothing crosses to the
    host.  A sequence depends on (seed, its global index) only."""
    import torch
    from . import _lib as L
    S, T, J = int(S), int(T), int(jitter)
    _check_strike(S, T, J, int(first_sequence))
    dev = torch.device(device)
    waves = torch.empty((S * T, 5), dtype=torch.float32, device=dev)
    nodes = torch.empty((S * T, 7, 8), dtype=torch.float32, device=dev)
    nnode = torch.empty((S * T,), dtype=torch.int32, device=dev)
    ident = torch.empty((S * T, 7), dtype=torch.int32, device=dev)
    if S == 0:                                              # empty tensors have no address to pass
        return waves, nodes, nnode, ident
    w0, n0, c0 = draw_params_device(S, seed, dev, count_range, first_sequence)
    with torch.cuda.device(dev):
        L.spnet_fake_espi_strike(w0.data_ptr(), n0.data_ptr(), c0.data_ptr(), int(first_sequence), S, T, int(seed) & 0xFFFFFFFF,
                                 J, waves.data_ptr(), nodes.data_ptr(), nnode.data_ptr(), ident.data_ptr(),
                                 torch.cuda.current_stream(dev).cuda_stream)
    return waves, nodes, nnode, ident


def strike_rows(nodes, nnode, ident):
    """Strike parameter arrays nodes [N,7,8], nnode [N], ident [N,7] (device tensors or host arrays) -> (rows float64
    [N,7,6], count int32 [N], ident int32 [N,7]) of the same kind in augmentation.pad_metadata's layout: the present slots
    moved to the front in slot order with their identities, zeros behind them.  The values rows_from_params gives, for
    parameters whose slots are no longer all at the front."""
    if hasattr(nodes, "is_cuda"):
        import torch
        j = torch.arange(7, device=nodes.device)
        valid = (nodes[..., 7] != 0) & (j[None, :] < nnode[:, None])
        order = torch.argsort((~valid).to(torch.int32), dim=1, stable=True)
        kept = torch.gather(valid, 1, order)
        rows = torch.gather(nodes[..., :6].trunc().double(), 1, order[..., None].expand(-1, -1, 6)) * kept[..., None]
        return (rows.contiguous(), valid.sum(1).to(torch.int32), (torch.gather(ident, 1, order) * kept).to(torch.int32))
    nodes, ident = np.asarray(nodes), np.asarray(ident)
    valid = (nodes[..., 7] != 0) & (np.arange(7)[None, :] < np.asarray(nnode)[:, None])
    order = np.argsort(~valid, axis=1, kind="stable")
    kept = np.take_along_axis(valid, order, 1)
    rows = np.take_along_axis(np.trunc(nodes[..., :6]).astype(np.float64), order[..., None], 1) * kept[..., None]
    return np.ascontiguousarray(rows), valid.sum(1).astype(np.int32), (np.take_along_axis(ident, order, 1) * kept).astype(np.int32)


def generate_strike_device(S, T, seed=0, jitter=0, first_sequence=0, count_range=(1, 7), device="cuda:0", noise=True,
                           want_u8=False, chunk=1024, size=None):
    """S strike sequences of T frames rasterised in HBM: strike_params_device, then generate_device on those parameters (the
    rasteriser, sensor model and resize unchanged).  -> (X float32 [S*T,H,W,1], (rows float64 [S*T,7,6], count int32 [S*T]),
    ident int32 [S*T,7][, uint8 frames]) device tensors; rows and ident are strike_rows'.  The sensor noise is keyed by the
    first FRAME, first_sequence * T, so another range of sequences gets other noise."""
    waves, nodes, nnode, ident = strike_params_device(S, T, seed, jitter, first_sequence, count_range, device)
    rows, count, ident = strike_rows(nodes, nnode, ident)
    if S == 0:
        import torch
        from .resize import _size
        OH, OW = (IM_H, IM_W) if size is None else _size(size)
        X = torch.empty((0, OH, OW, 1), dtype=torch.float32, device=device)
        U = torch.empty((0, OH, OW), dtype=torch.uint8, device=device)
        return (X, (rows, count), ident, U) if want_u8 else (X, (rows, count), ident)
    # labels="device" only keeps the slot-by-slot labels of generate_device off the host; they are NOT the movie's labels
    # (absent slots are zero rows there) and are dropped: rows, count and ident above are
    out = generate_device(S * T, seed, device, noise=noise, want_u8=want_u8, chunk=chunk, size=size,
                          params=(waves, nodes, nnode), first_frame=int(first_sequence) * int(T), labels="device")
    return (out[0], (rows, count), ident) + tuple(out[2:])


def generate_device(n, seed=0, device="cuda:0", noise=True, want_u8=False, chunk=1024, count_range=(1, 7),
                    bandpass_real=None, size=None, params="host", first_frame=0, labels="host", full_u8=None):
    """n frames rasterised directly in HBM (csrc/espi.hip): the SAME per-frame parameters as generate(n, seed)
    (so the labels are identical), pixels from the analytic device rasteriser, sensor noise / dropout from a
    counter-based RNG.  Returns (float32 device tensor [n,384,512,1] in [-1,1], label rows[, uint8 device tensor]).
    bandpass_real (directory of real 512x384 *.png, or a BandpassPool): the frames are band-pass mixed
    (augmentation.bandpass_mixup) -- the uint8 frame is the mixed one rounded as cv2.imwrite does, X is derived from it
    exactly as reading that PNG back would give.
    size (int or (OH, OW)): the frames are resized on the device as the input codec resizes them (PIL Lanczos, bit for
    bit: resize.py) -- X is [n,OH,OW,1] and the uint8 frames [n,OH,OW], exactly what writing the PNGs and reading them
    back through build_dataset at force_dim = size gives.  Labels stay in the 512x384 frame's coordinates.
    params: "host" (default) = the per-frame parameters of draw_params, the reference-ordered stream, drawn on the host
    frame by frame; "device" = drawn by draw_params_device for the GLOBAL frames first_frame .. first_frame + n - 1, chunk
    by chunk, the labels read back in one copy per chunk: the same distributions, other frames, and parameters / labels /
    noise-free pixels that do not depend on `chunk`.  The sensor noise keeps its seed of (seed, chunk start) as before
    (first_frame shifts the chunk start, so that another range of frames gets other noise); first_frame needs "device".
    params may also be the three parameter arrays themselves, (waves [n,5], nodes [n,7,8], nnode [n]) contiguous device
    tensors (generate_strike_device): they are rasterised as they are and the labels are read from them slot by slot.
    labels: "host" (default) = the label rows as Python lists; "device" (needs params="device") = rows_from_params' pair of
    device tensors instead, and no label crosses to the host.
    full_u8 (with size; a uint8 device tensor [n,384,512]): also receives the frames at their full size, as rasterised (and
    mixed), i.e. what the resize reads."""
    import torch
    from . import _lib as L
    given = isinstance(params, (tuple, list))
    if given:
        if len(params) != 3 or tuple(params[0].shape) != (n, 5) or tuple(params[1].shape) != (n, 7, 8) or \
                tuple(params[2].shape) != (n,) or not all(a.is_cuda and a.is_contiguous() for a in params):
            raise ValueError("generate_device: params as arrays are contiguous device tensors waves [n,5], nodes [n,7,8], nnode [n]")
        given, params = params, "device"
    if params not in ("host", "device"):
        raise ValueError("generate_device: params must be 'host', 'device' or three device tensors, got %r" % (params,))
    if labels not in ("host", "device") or (labels == "device" and params != "device"):
        raise ValueError("generate_device: labels must be 'host' or 'device' (which needs params='device'), got %r" % (labels,))
    if full_u8 is not None and (size is None or full_u8.dtype != torch.uint8 or tuple(full_u8.shape) != (n, IM_H, IM_W)
                                or not full_u8.is_contiguous()):
        raise ValueError("generate_device: full_u8 goes with size and is a contiguous uint8 tensor [%d,%d,%d]" % (n, IM_H, IM_W))
    if first_frame and params != "device":
        raise ValueError("generate_device: first_frame needs params='device' (the host stream is keyed by (n, seed))")
    dev = torch.device(device)
    mixer = bp = None
    if bandpass_real is not None:
        from .augmentation import BandpassPool
        mixer = BandpassPool.get(bandpass_real, IM_H, IM_W, dev).mixer
        bp = mixer.draw(n, seeds=bandpass_seeds(n, seed, first_frame))
    OH, OW = (IM_H, IM_W)
    if size is not None:
        from .resize import _size, resize_u8_device
        OH, OW = _size(size)
    X = torch.empty((n, OH, OW, 1), dtype=torch.float32, device=dev)
    U = torch.empty((n, OH, OW), dtype=torch.uint8, device=dev) if (want_u8 or (mixer is not None and size is None)) else None
    dev_labels = labels == "device"
    labels = []
    if dev_labels:
        rows_d = torch.empty((n, 7, 6), dtype=torch.float64, device=dev)
        count_d = torch.empty((n,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        if params == "device":
            wd, ndd, nnd = (a[lo:hi] for a in given) if given else \
                draw_params_device(hi - lo, seed, dev, count_range, first_frame + lo)
            if dev_labels:
                r, c = rows_from_params(ndd, nnd)
                rows_d[lo:hi].copy_(r)
                count_d[lo:hi].copy_(c)
            else:
                labels += labels_from_params(ndd, nnd)
        else:
            waves = np.zeros((hi - lo, 5), np.float32)
            nodes = np.zeros((hi - lo, 7, 8), np.float32)
            nn = np.zeros(hi - lo, np.int32)
            for k, s in enumerate(frame_seeds(n, seed)[lo:hi]):
                w, nd, _ = draw_params(s, count_range)
                waves[k] = w
                nn[k] = len(nd)
                for j, node in enumerate(nd):
                    nodes[k, j, :7] = node
                    nodes[k, j, 7] = 1.0
                labels.append([node[:6] for node in nd])
            wd, ndd, nnd = (torch.from_numpy(a).to(dev) for a in (waves, nodes, nn))
        if size is None:
            Xc, Uc = X[lo:hi], (U[lo:hi] if U is not None else None)
        else:               # the 384x512 uint8 frames of this chunk only; X / U receive them resized
            Xc = None
            Uc = full_u8[lo:hi] if full_u8 is not None else torch.empty((hi - lo, IM_H, IM_W), dtype=torch.uint8, device=dev)
        L.spnet_fake_espi(wd.data_ptr(), ndd.data_ptr(), nnd.data_ptr(), hi - lo, IM_H, IM_W,
                          (seed * 2654435761 + (first_frame + lo) * 97 + 12345) & 0xFFFFFFFF, int(bool(noise)), L.ptr(Xc),
                          L.ptr(Uc), st)
        if mixer is not None:
            mixer.apply({k: v[lo:hi] for k, v in bp.items()}, Uc, out_u8=Uc)
            if size is None:
                L.spnet_u8_to_input(Uc.data_ptr(), Xc.data_ptr(), (hi - lo) * IM_H * IM_W, st)
        if size is not None:
            resize_u8_device(Uc, (OH, OW), out_f=X[lo:hi], out_u8=None if U is None else U[lo:hi])
        torch.cuda.current_stream(dev).synchronize()       # wd / ndd / nnd (/ Uc) are freed on return
    if dev_labels:
        labels = (rows_d, count_d)
    return (X, labels, U) if want_u8 else (X, labels)


def targets_from_labels(labels, pred_grid=(6, 6, 2)):
    """Label rows of a chunk of frames -> (Y float32 [B, prod(pred_grid) * 8], overflow bool [B]): the file path's row
    processing (a/b swap with +90 degrees, rings > 0, sort by (cx, cy)), true_to_pred_grid and norm_Y, vectorised
    (augmentation._encode_targets) and bit-identical to writing the rows with rows_to_csv and loading the CSV.  overflow
    marks the frames where a third ellipse falls into one grid cell; their targets hold the two that fit."""
    from .augmentation import _encode_targets, pad_metadata
    rows, count = pad_metadata(list(labels))
    Y, overflow = _encode_targets(rows, count, tuple(pred_grid))
    return np.ascontiguousarray(Y, dtype=np.float32), overflow


class FakeStream:
    """An endless supply of fake-ESPI training frames: epoch e is the n global frames e*n .. e*n + n - 1 of the device
    parameter stream (generate_device(params="device")), with their normalised grid targets.  Nothing is read from or
    written to disk.  size: None = native 384x512 frames (model_type 'big'), 331 = the default layout (resized on the device
    as the input codec resizes).  targets: "device" (default) = the labels stay in HBM and the targets come from
    spnet_encode_targets (augmentation.encode_targets_device; the drawn angles are whole degrees, so the same bits); "host"
    = the labels are read back and encoded in numpy (targets_from_labels), the oracle of the former."""

    def __init__(self, n, seed=0, device="cuda:0", size=None, count_range=(1, 7), pred_grid=(6, 6, 2), bandpass_real=None,
                 chunk=1024, targets="device"):
        if targets not in ("device", "host"):
            raise ValueError("FakeStream: targets must be 'device' or 'host', got %r" % (targets,))
        self.targets = targets
        self.U_full = self.rows = self.count = None         # epoch(keep_u8=True): full-size frames and device label rows
        self.n, self.seed, self.device, self.size = int(n), int(seed), device, size
        self.count_range, self.pred_grid, self.bandpass_real, self.chunk = tuple(count_range), tuple(pred_grid), bandpass_real, chunk
        if size is None:
            self.frame_shape = (IM_H, IM_W, 1)
        else:
            from .resize import _size
            self.frame_shape = tuple(_size(size)) + (1,)
        from . import config as cf
        self.n_targets = int(np.prod(self.pred_grid)) * cf.vars_per_pred
        self.overflowed = 0                 # frames of the last epoch() with a third ellipse in one grid cell

    def frames(self, first_frame, n, want_u8=False, **kw):
        """generate_device for the global frames first_frame .. first_frame + n - 1 of this stream."""
        return generate_device(n, self.seed, self.device, count_range=self.count_range, bandpass_real=self.bandpass_real,
                               size=self.size, chunk=self.chunk, params="device", first_frame=first_frame, want_u8=want_u8, **kw)

    def epoch(self, e, out_X=None, out_Y=None, verbose=True, keep_u8=False):
        """Fills out_X [n,H,W,1] float32 and out_Y [n, n_targets] float32 (device tensors; allocated when None) with the
        frames and targets of epoch e; returns (out_X, out_Y).  A frame with a third ellipse in one grid cell keeps the two
        that fit (the file path would assert); their number is kept in self.overflowed (with targets="device": the
        epoch's one scalar read back) and printed.
        keep_u8 (needs targets="device"): the epoch's full-size 384x512 uint8 frames and its label rows stay in self.U_full
        [n,384,512], self.rows [n,7,6] float64 and self.count [n] int32 -- the same three tensors every epoch, rewritten
        in place: what a DeviceWarper built on them warps."""
        import torch
        if keep_u8 and self.targets != "device":
            raise ValueError("FakeStream.epoch: keep_u8 needs targets='device' (the label rows stay on the device)")
        kw = {}
        if keep_u8:
            if self.U_full is None:
                self.U_full = torch.empty((self.n, IM_H, IM_W), dtype=torch.uint8, device=self.device)
            kw = dict(full_u8=self.U_full) if self.size is not None else dict(want_u8=True)
        if self.targets == "device":
            from .augmentation import encode_targets_device
            X, (rows, count), *U = self.frames(int(e) * self.n, self.n, labels="device", **kw)
            Yd, flags = encode_targets_device(rows, count, self.pred_grid)
            self.overflowed = int((flags != 0).sum())
            if keep_u8:
                if U:                       # native frames: the uint8 frames themselves
                    self.U_full.copy_(U[0])
                if self.rows is None:
                    self.rows, self.count = rows, count
                else:
                    self.rows.copy_(rows)
                    self.count.copy_(count)
        else:
            X, labels = self.frames(int(e) * self.n, self.n)
            Y, overflow = targets_from_labels(labels, self.pred_grid)
            self.overflowed = int(overflow.sum())
            Yd = torch.from_numpy(Y).to(X.device)
        if verbose:
            print("   Fresh fake-ESPI frames: epoch %d = frames %d .. %d; %d frames with a third ellipse in one grid cell keep "
                  "the two that fit" % (e, int(e) * self.n, int(e) * self.n + self.n - 1, self.overflowed))
        if out_X is None:
            out_X = X
        else:
            out_X.copy_(X.reshape(out_X.shape))
        if out_Y is None:
            out_Y = Yd
        else:
            out_Y.copy_(Yd)
        return out_X, out_Y


def rows_to_csv(rows):
    if not rows:
        return "0,0,0,0,0,0.0"
    return "\n".join("{0},{1},{2},{3},{4},{5}".format(*r) for r in rows)


def gpu_may_be_live():
    """True when this process may already hold a HIP context, i.e. when fork() is unsafe: torch has initialised the
    GPU, or a profiler's preloaded tool library has (rocprofv3 initialises the runtime before Python starts, and
    torch.cuda.is_initialized() stays False then)."""
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
        return True
    env = os.environ
    if any(k.startswith(("ROCPROFILER_", "ROCPROF_", "ROCP_")) for k in env):
        return True
    return any(t in env.get(k, "") for k in ("LD_PRELOAD", "HSA_TOOLS_LIB") for t in ("rocprof", "roctracer", "rocprofiler"))


def generate(n, seed=0, workers=None):
    """n frames -> (uint8 [n,384,512], list of label rows).  Deterministic in (n, seed)."""
    seeds = frame_seeds(n, seed)
    workers = workers or min(os.cpu_count() or 1, 16)
    # Worker processes are FORKED: safe only while this process has not initialised the GPU (a forked copy of a
    # HIP-initialised, multi-threaded process crashes or hangs).  Afterwards: small sets serially, large ones from
    # freshly spawned interpreters.
    ctx = None
    if workers > 1 and n >= 16:
        import multiprocessing
        if not gpu_may_be_live():
            ctx = multiprocessing.get_context("fork")
        elif n >= 512:
            ctx = multiprocessing.get_context("spawn")
    if ctx is not None:
        p = ctx.Pool(workers)
        try:
            res = p.map(gen_frame, seeds, chunksize=max(1, n // (workers * 4)))
        finally:                     # let the workers exit normally (Pool.__exit__ would terminate() = SIGTERM them)
            p.close()
            p.join()
    else:
        res = [gen_frame(s) for s in seeds]
    X = np.stack([r[0] for r in res])
    return X, [r[1] for r in res]


def to_network_input(X_u8):
    """uint8 [n,H,W] -> float32 [n,H,W,1] in [-1,1] exactly as load_X_one_proc scales (utils.py:340-342)."""
    x = X_u8.astype(np.float32) / 255.0
    x -= 0.5
    x *= 2.0
    return x[..., None]


def write_dataset(path, n, seed=0, start=0, bandpass_real=None, bp_path=None, chunk=256):
    """steelpan_NNNNNNN.png + .csv pairs under `path` (the layout build_dataset reads).  bandpass_real (directory of real
    512x384 *.png) with bp_path: also the band-pass mixed frames, steelpan_NNNNNNN_bp.png + steelpan_NNNNNNN_bp.csv
    (the same labels) under bp_path -- a dataset of its own: the reference writes the _bp.png beside the frame
    (gen_fake_espi.py:269-271), which build_dataset's PNG / CSV count assertion rejects."""
    if (bandpass_real is None) != (bp_path is None):
        raise ValueError("write_dataset: bandpass_real and bp_path go together")
    os.makedirs(path, exist_ok=True)
    X, labels = generate(n, seed)
    for i in range(n):
        stem = os.path.join(path, "steelpan_" + str(start + i).zfill(7))
        Image.fromarray(X[i]).save(stem + ".png")
        with open(stem + ".csv", "w") as f:
            f.write(rows_to_csv(labels[i]))
    if bandpass_real is not None:
        import torch
        from .augmentation import BandpassPool
        os.makedirs(bp_path, exist_ok=True)
        mixer = BandpassPool.get(bandpass_real, IM_H, IM_W).mixer
        bp = mixer.draw(n, seeds=bandpass_seeds(n, seed))
        dev = mixer.pool.images.device
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            u = torch.from_numpy(X[lo:hi]).to(dev)
            mixer.apply({k: v[lo:hi] for k, v in bp.items()}, u, out_u8=u)
            mixed = u.cpu().numpy()
            for i in range(lo, hi):
                stem = os.path.join(bp_path, "steelpan_" + str(start + i).zfill(7) + "_bp")
                Image.fromarray(mixed[i - lo]).save(stem + ".png")
                with open(stem + ".csv", "w") as f:
                    f.write(rows_to_csv(labels[i]))
    return X, labels
