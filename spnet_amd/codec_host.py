"""The host side that the device codecs (png.py, jpeg.py) share: the thread pool of at most 16 threads that reads, parses and
writes files, the one staged host-to-device copy of a call's small arrays, the file writer, the default path's decode of one
file, and decode_batch, the skeleton of a decode call (host-only files first, one size per call, the status download as the
only synchronisation, rejected files retried on the host, one stacked fallback upload).  A codec supplies its parse, its
channels_of and its launch (see decode_batch); this module imports neither codec."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

MAX_THREADS = 16                # the CPU allowance of a process on a shared machine; nothing is forked


def pool_size(threads, jobs):
    return max(1, min(MAX_THREADS, int(threads), jobs))


def map_pool(fn, items, threads=MAX_THREADS):
    """[fn(item)] in order, on a thread pool of this process (pool_size threads); no items: [] and no pool."""
    items = list(items)
    if not items:
        return []
    with ThreadPoolExecutor(max_workers=pool_size(threads, len(items))) as pool:
        return list(pool.map(fn, items))


def read_file(path):
    with open(path, "rb") as f:
        return f.read()


def host_frame(source, channels):
    """The default path's decode of one file (spnet_amd.utils._load_one's Pillow call decides what a damaged file is):
    channel 0 of convert("RGB") as [H,W], or every channel as the file holds them, [H,W,C]."""
    import io
    from PIL import Image
    f = source if isinstance(source, (str, os.PathLike)) else io.BytesIO(source)
    if channels == "first":
        return np.asarray(Image.open(f).convert("RGB"), dtype=np.uint8)[:, :, 0]
    arr = np.asarray(Image.open(f))
    if arr.dtype != np.uint8:
        raise ValueError('png: channels="all" holds 8-bit samples, this file decodes to %s' % arr.dtype)
    return arr.reshape(arr.shape[0], arr.shape[1], -1)


def stage(parts, device, pinned, align):
    """The host arrays `parts` as ONE host-to-device copy: laid out back to back in their order, each padded to `align`
    bytes, in one host buffer (pinned: page-locked, and the copy is non_blocking; else pageable and blocking).  Returns (the
    uint8 device tensor that owns the bytes, the byte offset of every part in it, the host buffer: the caller keeps it alive
    until the copy has been waited for)."""
    import torch
    parts = [np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in parts]
    starts, total = [], 0
    for p in parts:
        starts.append(total)
        total += (p.size + align - 1) // align * align
    host = torch.empty((max(total, 1),), dtype=torch.uint8)
    if pinned:
        host = host.pin_memory()
    buf = host.numpy()
    for s, p in zip(starts, parts):
        buf[s:s + p.size] = p
    return host.to(device, non_blocking=pinned), starts, host


def write_files(paths, n, encode, threads, pool, name):
    """n files written to `paths` by a thread pool (pool: a caller's ThreadPoolExecutor, left open; None: one of our own of
    pool_size threads).  ValueError unless there are n paths; only then encode() runs, once, and returns pieces_of: file k
    is the byte pieces pieces_of(k), written in order.  Returns the size of every file."""
    paths = list(paths)
    if len(paths) != n:
        raise ValueError("%s: %d frames, %d paths" % (name, n, len(paths)))
    if n == 0:
        return []
    pieces_of = encode()

    def job(k):
        size = 0
        with open(paths[k], "wb") as f:
            for piece in pieces_of(k):
                f.write(piece)
                size += len(piece)
        return size

    if pool is not None:
        return list(pool.map(job, range(n)))
    with ThreadPoolExecutor(max_workers=pool_size(threads, n)) as own:
        return list(own.map(job, range(n)))


def decode_batch(infos, sources, device, channels, return_info, name, channels_of, launch, info_type=list):
    """The decode call of codec `name` over parsed files: infos[k] has .device (False: the host decodes sources[k]),
    .height and .width; channels_of(info) is the channel count of a file the device decodes.
    launch(idx, shape, out, device) enqueues the codec's kernels for the files idx (those with .device, possibly none), all
    of one `shape` ([H,W] or [H,W,C]), and returns (a list of (indices, status, got, keepalive), extras): status an int32
    device tensor [len(indices)], got the frames of `indices` (`out` itself where the launch filled it in place), keepalive
    whatever has to outlive the launches.  Nothing is synchronised before every launch is enqueued.
    Returns the uint8 device tensor [N,H,W] / [N,H,W,C]; with return_info also the status array and
    info_type(sorted indices of the files the host decoded, *extras)."""
    import torch
    if channels not in ("first", "all"):
        raise ValueError('%s: channels is "first" or "all", got %r' % (name, channels))
    if not torch.cuda.is_available():
        raise RuntimeError("%s: decode_%s_device decodes on the GPU (there is no CPU decoder here)" % (name, name))
    device = torch.device("cuda" if device is None else device)
    N = len(infos)
    status = np.zeros(N, np.int32)
    host = [k for k in range(N) if not infos[k].device]
    host_frames = {k: host_frame(sources[k], channels) for k in host}          # raises what the default path raises

    def shape_of(k):
        if k in host_frames:
            return host_frames[k].shape
        return (infos[k].height, infos[k].width) + ((channels_of(infos[k]),) if channels == "all" else ())

    if N == 0:
        out = torch.empty((0, 0, 0) if channels == "first" else (0, 0, 0, 0), dtype=torch.uint8, device=device)
        return (out, status, info_type()) if return_info else out
    shape = shape_of(0)
    for k in range(1, N):
        if shape_of(k) != shape:
            which = sources[k] if isinstance(sources[k], (str, os.PathLike)) else "file %d" % k
            raise ValueError("%s: %s is %s, the files before it are %s (one call decodes files of one size)"
                             % (name, which, "x".join(str(v) for v in shape_of(k)), "x".join(str(v) for v in shape)))
    out = torch.empty((N,) + tuple(shape), dtype=torch.uint8, device=device)
    pending, extras = launch([k for k in range(N) if infos[k].device], tuple(shape), out, device)
    for idx, st, got, _ in pending:
        status[idx] = st.cpu().numpy()           # the D2H copy of the status: the only synchronisation
        if got is not out:
            out[torch.as_tensor(idx, device=device)] = got
    failed = [k for k in range(N) if status[k] != 0]
    for k in failed:
        host_frames[k] = host_frame(sources[k], channels)       # a corrupt file raises here what it raises today
        if host_frames[k].shape != tuple(shape):
            raise ValueError("%s: file %d decodes to %s on the host, %s was expected" % (name, k, host_frames[k].shape, shape))
    fallback = sorted(host_frames)
    if fallback:
        up = torch.from_numpy(np.stack([host_frames[k] for k in fallback])).to(device)
        out[torch.as_tensor(fallback, device=device)] = up
    return (out, status, info_type(fallback, *extras)) if return_info else out
