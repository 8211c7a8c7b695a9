"""Data / target codec and output helpers -- the host-side surface of the reference's spnet/utils.py.

  grid codec      setup_means_and_ranges, true_to_pred_grid, norm_Y, denorm_Y   (utils.py:144-244)
  metadata        parse_meta_file, build_Y                                      (utils.py:260-320)
                  read_metadata (raw rows for the warps)                        (augment_preproc.py:25-38)
  frames          build_X (PNG -> float32 [N,H,W,1] in [-1,1]), build_dataset   (utils.py:325-482)
  outputs         cleanup_antinode_vars, show_pred_ellipses (overlay PNGs + hawley_spnet.csv)
                                                                                (utils.py:56-137)
OpenCV is not available on the target image: overlays are drawn with PIL (anti-aliased polygon
outline instead of cv2.ellipse with shift=10), so the PNGs are visually equivalent, not bit-identical;
the CSV rows are computed exactly as the reference does.
"""
import errno
import glob
import math
import os
import random
from functools import partial
from multiprocessing import cpu_count
from operator import itemgetter

import numpy as np
import pandas as pd
from PIL import Image, ImageDraw

from . import config as cf

orig_img_dims = [512, 384]
means = []
ranges = []


def make_sure_path_exists(path):
    try:
        os.makedirs(path)
    except OSError as exc:
        if exc.errno != errno.EEXIST:
            raise


# ----------------------------------------------------------------------------- grid codec
def setup_means_and_ranges(pred_shape):
    """Per-cell means / ranges / 'blank' defaults of the predictor grid (utils.py:144-176).
    NOTE the first grid axis indexes x (image width), the second y."""
    global means, ranges
    cx_min, cy_min, cx_max, cy_max = 40, 40, 470, 350
    nx, ny = int(pred_shape[0]), int(pred_shape[1])
    xbinsize = int((cx_max - cx_min) / nx)
    ybinsize = int((cy_max - cy_min) / ny)
    shape = tuple(int(v) for v in pred_shape)
    gridmeans = np.zeros(shape, dtype=cf.dtype)
    gridranges = np.zeros(shape, dtype=cf.dtype)
    gridYi = np.zeros(shape, dtype=cf.dtype)
    xs = np.arange(nx) * xbinsize + cx_min + xbinsize / 2
    ys = np.arange(ny) * ybinsize + cy_min + ybinsize / 2
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    for slot in range(shape[2]):
        #                      cx   cy   a             b             cos2t sin2t noobj rings
        gridYi[:, :, slot, 0], gridYi[:, :, slot, 1] = gx, gy
        gridYi[:, :, slot, 2:] = [xbinsize / 2, ybinsize / 2, -1, 0, 1, 0]
        gridmeans[:, :, slot, 0], gridmeans[:, :, slot, 1] = gx, gy
        gridmeans[:, :, slot, 2:] = [xbinsize / 2, ybinsize / 2, 0, 0, 0, 5]
        gridranges[:, :, slot, :] = [xbinsize, ybinsize, xbinsize, ybinsize, 2, 2, 1, 10]
    means = gridmeans.flatten()
    ranges = gridranges.flatten()
    return cx_min, cy_min, cx_max, cy_max, xbinsize, ybinsize, gridYi


def norm_Y(Y, set_means_ranges=False):
    return (Y - means) / ranges


def denorm_Y(normY):
    return normY * ranges + means


def true_to_pred_grid(true_arr, pred_shape, num_classes=11, img_filename=None):
    """Scatter one image's ellipses [cx,cy,a,b,cos2t,sin2t,noobj,rings] over the grid of predictors
    (utils.py:191-244): cell = clip(int((c - 40)/bin)), next free slot, AssertionError on overflow."""
    cx_min, cy_min, _, _, xbinsize, ybinsize, gridYi = setup_means_and_ranges(pred_shape)
    true_arr = np.asarray(true_arr)
    taken = np.zeros(gridYi.shape[0:2], dtype=int)
    if true_arr.ndim < 2:
        return gridYi
    for row in true_arr:
        ix = min(max(int((row[0] - cx_min) / xbinsize), 0), int(pred_shape[0]) - 1)
        iy = min(max(int((row[1] - cy_min) / ybinsize), 0), int(pred_shape[1]) - 1)
        assert taken[ix, iy] < pred_shape[2], \
            "grid cell (%d,%d) already holds %d ellipses (%s)" % (ix, iy, taken[ix, iy], img_filename)
        gridYi[ix, iy, taken[ix, iy]] = row
        taken[ix, iy] += 1
    return gridYi


def add_to_stack(a, b):
    return [b] if a is None else a + [b]


def nearest_multiple(a, b):
    return int(a / b) * b


def parse_meta_file(meta_filename):
    """CSV rows cx,cy,a,b,angle,rings -> sorted list of [cx,cy,a,b,cos2t,sin2t,0,rings] (utils.py:260-286)."""
    try:
        df = pd.read_csv(meta_filename, header=None, names=['cx', 'cy', 'a', 'b', 'angle', 'rings'])
    except pd.errors.EmptyDataError:
        return []
    df.drop_duplicates(inplace=True)
    out = []
    for cx, cy, a, b, angle, rings in df.itertuples(index=False):
        angle = float(angle)
        if b > a:
            a, b, angle = b, a, angle + 90
        if rings > 0.0:
            t = 2 * np.deg2rad(angle)
            out.append([cx, cy, a, b, np.cos(t), np.sin(t), 0, rings])
    return sorted(out, key=itemgetter(0, 1))


def read_metadata(meta_filename):
    """CSV rows cx,cy,a,b,angle,rings as augment_preproc.py:25-38 reads them for warping: duplicates dropped, angle as
    float, sorted by (cx, cy); no a/b swap and no ring filter (parse_meta_file applies those when the file is loaded)."""
    try:
        df = pd.read_csv(meta_filename, header=None, names=['cx', 'cy', 'a', 'b', 'angle', 'rings'])
    except pd.errors.EmptyDataError:
        return []
    df.drop_duplicates(inplace=True)
    arrs = []
    for _, row in df.iterrows():        # (iterrows: a row's values share one dtype, as in the reference)
        arrs.append([row['cx'], row['cy'], row['a'], row['b'], float(row['angle']), row['rings']])
    return sorted(arrs, key=itemgetter(0, 1))


def build_Y(total_load, meta_file_list, img_file_list, pred_grid=[6, 6, 2], set_means_ranges=False):
    pred_shape = np.array([pred_grid[0], pred_grid[1], pred_grid[2], cf.vars_per_pred], dtype=int)
    num_outputs = int(np.prod(pred_shape))
    Y = np.zeros([total_load, num_outputs], dtype=cf.dtype)
    for i in range(total_load):
        if 0 == i % 5000:
            print("      Reading metadata file i =", i, "/", total_load, ":", meta_file_list[i])
        rows = np.array(parse_meta_file(meta_file_list[i]))
        Y[i, :] = true_to_pred_grid(rows, pred_shape, img_filename=img_file_list[i]).flatten()
    if total_load == 0:
        setup_means_and_ranges(pred_shape)
    return norm_Y(Y, set_means_ranges=set_means_ranges), pred_shape


# ----------------------------------------------------------------------------- frames
def _load_one(force_dim, grayscale, filename, as_uint8=False):
    img = Image.open(filename).convert("RGB")
    if force_dim is not None:
        img = img.resize((force_dim, force_dim), Image.LANCZOS)     # PIL.Image.ANTIALIAS of the reference
    if as_uint8:           # grey levels as decoded (channel 0); Model.predict scales them on the device
        return np.asarray(img, dtype=np.uint8)[:, :, 0:1]
    arr = np.asarray(img, dtype=np.float32)
    arr = (arr / 255.0 - 0.5) * 2.0
    return arr[:, :, 0:1] if grayscale else arr


def build_X(total_load, img_file_list, force_dim=224, grayscale=False, as_uint8=False, device_resize=False,
            device_decode=False, frames=None):
    """PNG -> X float32 [N,H,W,C] scaled to [-1,1]; channel 0 only when grayscale (utils.py:325-421).
    as_uint8 (additive, grayscale only): keep the decoded grey levels, uint8 [N,H,W,1]; Model.predict applies the
    same scaling on the device (bit-identical), and the frames cross PCIe as bytes.
    device_resize (additive, with as_uint8): the grey levels are kept at the files' own size and force_dim is left to
    Model.predict(X, resize=True), which resizes on the device exactly as PIL does here (spnet_amd/resize.py).
    device_decode (additive, with as_uint8; implies device_resize): the files' bytes are uploaded as they are and decoded
    on the GPU (spnet_amd.jpeg.read_frames_device: PNG files by spnet_amd.png.read_png_device, JPEG files by
    read_jpeg_device); X is then a uint8 DEVICE tensor [N,h,w,1] at the files' own size, with the same grey levels.
    frames (additive, with as_uint8): uint8 frames that are already in device memory, [N,h,w] or [N,h,w,1] (the frames of
    a movie, spnet_amd.jpeg.MjpegReader.read_device): X is the first total_load of them as [N,h,w,1]; no file is opened."""
    print("      Reading images and assigning as input X...")
    if as_uint8 and not grayscale:
        raise ValueError("as_uint8 is for grayscale input (model_type 'big' / 'monolithic')")
    if frames is not None:
        if not as_uint8:
            raise ValueError("frames needs as_uint8=True (they are 8-bit grey levels)")
        if frames.dim() not in (3, 4) or (frames.dim() == 4 and int(frames.shape[3]) != 1) or int(frames.shape[0]) < total_load:
            raise ValueError("frames are at least %d grey frames [N,h,w] or [N,h,w,1], got %s"
                             % (total_load, tuple(frames.shape)))
        X = frames[0:total_load]
        X = X.unsqueeze(-1) if X.dim() == 3 else X
        return X, tuple(int(v) for v in X.shape[1:])
    if device_decode:
        if not as_uint8:
            raise ValueError("device_decode needs as_uint8=True (the device decodes to 8-bit grey levels)")
        from .jpeg import read_frames_device
        X = read_frames_device(list(img_file_list[0:total_load])).unsqueeze(-1)
        return X, tuple(int(v) for v in X.shape[1:])
    if device_resize:
        if not as_uint8:
            raise ValueError("device_resize needs as_uint8=True (the device resizes 8-bit grey levels)")
        force_dim = None
    first = _load_one(force_dim, grayscale, img_file_list[0], as_uint8)
    img_dims = first.shape
    X = np.zeros((total_load,) + img_dims, dtype=np.uint8 if as_uint8 else cf.dtype)
    worker = partial(_load_one, force_dim, grayscale, as_uint8=as_uint8)
    nproc = min(cpu_count(), max(1, total_load // 64))
    if nproc > 1:
        # forked workers are only safe while this process has not initialised the GPU (train_spnet.py evaluates and
        # predicts after training in one process): afterwards load from freshly spawned interpreters
        import multiprocessing
        from .fake_espi import gpu_may_be_live
        gpu_live = gpu_may_be_live()
        pool = multiprocessing.get_context("spawn" if gpu_live else "fork").Pool(nproc)
        try:
            for i, arr in enumerate(pool.imap(worker, img_file_list[0:total_load], chunksize=32)):
                X[i] = arr
        finally:
            pool.close()
            pool.join()
    else:
        for i in range(total_load):
            X[i] = worker(img_file_list[i])
    return X, img_dims


def build_dataset(path="Train/", load_frac=1.0, set_means_ranges=False, pred_grid=[6, 6, 2], batch_size=None,
                  shuffle=True, device_decode=False):
    """X, Y, img_file_list, pred_shape for one directory of PNG + same-stem CSV (utils.py:425-482)."""
    if cf.model_type == 'simple':
        grayscale, force_dim = False, 224
    elif cf.model_type == 'big':
        grayscale, force_dim = True, None        # native 384x512 frames (predict_spnet.py:47-55)
    else:
        grayscale, force_dim = True, 331
    print("Loading data from", path, ", fraction =", load_frac)
    img_file_list = sorted(glob.glob(path + '*.png'))
    meta_file_list = sorted(glob.glob(path + '*' + cf.meta_extension))
    assert len(img_file_list) == len(meta_file_list), \
        "Error: len(img_file_list) = %d but len(meta_file_list) = %d" % (len(img_file_list), len(meta_file_list))
    if shuffle and img_file_list:
        pairs = list(zip(img_file_list, meta_file_list))
        random.shuffle(pairs)
        img_file_list, meta_file_list = zip(*pairs)
    total_files = len(img_file_list)
    total_load = int(total_files * load_frac)
    if batch_size is not None:
        total_load = nearest_multiple(total_load, batch_size)
    print("      Total files = ", total_files, ", going to load total_load = ", total_load)
    Y, pred_shape = build_Y(total_load, meta_file_list, img_file_list, pred_grid=pred_grid,
                            set_means_ranges=set_means_ranges)
    if device_decode:          # (additive) uint8 device frames at the files' own size: Model.predict(X, resize=True)
        if not grayscale:
            raise ValueError("device_decode is for grayscale input (model_type 'big' / 'monolithic')")
        X, _ = build_X(total_load, img_file_list, force_dim=force_dim, grayscale=True, as_uint8=True, device_decode=True)
    else:
        X, _ = build_X(total_load, img_file_list, force_dim=force_dim, grayscale=grayscale)
    return X, Y, img_file_list, pred_shape


# ----------------------------------------------------------------------------- outputs
def cleanup_antinode_vars(Y_subarr):
    """(cx,cy,a,b,angle_deg,noobj,rings) with integer geometry and angle in (0,180] (utils.py:56-64)."""
    cx, cy, a, b, cos2t, sin2t, noobj, rings = Y_subarr
    cx, cy, a, b, noobj = [int(round(v)) for v in (cx, cy, a, b, noobj)]
    angle = np.rad2deg(np.arctan2(sin2t, cos2t) / 2.0)
    angle = angle if angle > 0 else angle + 180
    return cx, cy, a, b, angle, noobj, rings


def ellipse_polygon(center, axes, angle_deg, n=72):
    """Vertices of the ellipse the reference draws with cv2.ellipse(..., -angle, ...) (utils.py:35-53):
    image y points down, so a positive annotation angle rotates counter-clockwise on screen."""
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    th = np.deg2rad(-angle_deg)
    x = axes[0] * np.cos(t)
    y = axes[1] * np.sin(t)
    return np.stack([center[0] + x * np.cos(th) - y * np.sin(th), center[1] + x * np.sin(th) + y * np.cos(th)], 1)


def draw_ellipse(img, center, axes, angle, startAngle=0, endAngle=360, color=(0,), thickness=2, **_):
    """Draw on a PIL image (in place).  thickness < 0 fills.  `color` is BGR like the reference's."""
    pts = [tuple(p) for p in ellipse_polygon(center, axes, angle)]
    rgb = tuple(color[::-1]) if len(color) == 3 else color[0]
    d = ImageDraw.Draw(img)
    if thickness < 0:
        d.polygon(pts, fill=rgb)
    else:
        d.line(pts + [pts[0]], fill=rgb, width=int(thickness), joint="curve")
    return img


def show_pred_ellipses(Yt, Yp, file_list, num_draw=40, log_dir='./logs/', ind_extra=None, out_csv=None,
                       show_true=True, verbosity=0, png="host", png_chunk=64, draw="host", device_decode=False,
                       jpeg_quality=90, movie=None, movie_fps=5.0, frames=None):
    """Overlay PNGs steelpan_pred_%05d.png and the zooniverse-style CSV (cx,cy,file,rings,a,b,angle)
    from de-normalised true / predicted grids (utils.py:67-137).  png = "host": every overlay is saved by Pillow as it is
    drawn; "device" (additive): the drawn RGB overlays are collected png_chunk at a time, uploaded, encoded on the GPU
    (spnet_amd.png) and written by a thread pool -- the same pixels, file names and CSV rows, other file bytes; "device-lz":
    the same with the encoder's LZ77 stage on (smaller files); "device-jpeg" (additive): steelpan_pred_%05d.jpg instead,
    baseline JPEG of quality jpeg_quality encoded on the GPU (spnet_amd.jpeg) -- lossy, the same file numbers and CSV rows.
    movie (additive): an spnet_amd.jpeg.MjpegWriter, or a path (a Motion-JPEG AVI of movie_fps frames per second and
    quality jpeg_quality is written there and closed at the end): every drawn frame is also appended to it, in j order,
    whatever png is.
    draw = "host": Pillow draws; "device" (additive): the loop only plans (spnet_amd.overlay.plan_overlays), the frames
    are loaded png_chunk at a time -- by the device decoder with device_decode, else by Pillow and one upload per chunk --
    and one HIP launch per chunk draws them: the same file names and CSV rows, the same pixels away from outline edges
    (spnet_amd/overlay.py has the rule).
    frames (additive, with draw="device"): the frames themselves, a uint8 device tensor [N,H,W] (grey) or [N,H,W,3] in the
    order of file_list (the frames of a movie, spnet_amd.jpeg.MjpegReader.read_device); file_list then only names them and
    no file is opened."""
    if png not in ("host", "device", "device-lz", "device-jpeg"):
        raise ValueError('show_pred_ellipses: png is "host", "device", "device-lz" or "device-jpeg", got %r' % (png,))
    if draw not in ("host", "device"):
        raise ValueError('show_pred_ellipses: draw is "host" or "device", got %r' % (draw,))
    if draw == "host" and device_decode:
        raise ValueError('show_pred_ellipses: device_decode loads the frames for draw="device"')
    if draw == "host" and frames is not None:
        raise ValueError('show_pred_ellipses: frames= are device frames for draw="device"')
    sink = _OverlaySink(png, jpeg_quality, movie, movie_fps)
    try:
        if draw == "device":
            return _show_pred_ellipses_device(Yt, Yp, file_list, num_draw, log_dir, out_csv, show_true, png, png_chunk,
                                              device_decode, sink, frames)
        return _show_pred_ellipses_host(Yt, Yp, file_list, num_draw, log_dir, out_csv, show_true, png, png_chunk, sink)
    finally:
        sink.close()


class _OverlaySink:
    """Where drawn overlays that are in device memory go: the files of png = "device" / "device-lz" / "device-jpeg" and the
    movie.  A movie given as a path is opened at the first frames (their size is the movie's) and closed by close()."""

    def __init__(self, png, jpeg_quality, movie, movie_fps):
        self.png, self.quality, self.fps = png, jpeg_quality, movie_fps
        self.extension = ".jpg" if png == "device-jpeg" else ".png"
        self.movie = None if isinstance(movie, (str, os.PathLike)) else movie
        self.movie_path = movie if self.movie is None else None
        self.wants_device_frames = png != "host" or movie is not None

    def write(self, frames, paths):
        """frames: uint8 device tensor [n,H,W,3]; paths: the files of png != "host"."""
        if self.png == "device-jpeg":
            from .jpeg import write_jpeg_device
            write_jpeg_device(frames, paths, quality=self.quality)
        elif self.png != "host":
            from .png import write_png_device
            write_png_device(frames, paths, lz77=self.png == "device-lz")
        if self.movie is None and self.movie_path is not None:
            from .jpeg import MjpegWriter
            self.movie = MjpegWriter(self.movie_path, int(frames.shape[2]), int(frames.shape[1]), fps=self.fps,
                                     channels=3, quality=self.quality)
        if self.movie is not None:
            self.movie.add(frames)

    def close(self):
        if self.movie_path is not None and self.movie is not None:
            self.movie.close()


def _show_pred_ellipses_host(Yt, Yp, file_list, num_draw, log_dir, out_csv, show_true, png, png_chunk, sink):
    """show_pred_ellipses(draw="host"): Pillow draws."""
    m = Yt.shape[0]
    num_draw = min(num_draw, m, len(file_list))
    if out_csv is not None:
        open(out_csv, "w").close()
    n_pred = int(Yt[0].size / cf.vars_per_pred)
    held = []                # png != "host" or a movie: (overlay as uint8 [H,W,3], its file), frames of one size

    def flush():
        if held:
            import torch
            if not torch.cuda.is_available():
                raise RuntimeError('show_pred_ellipses: png="device..." and movie= encode on the GPU (no CPU fallback)')
            sink.write(torch.from_numpy(np.stack([h[0] for h in held])).cuda(), [h[1] for h in held])
            held.clear()

    for j in range(num_draw):
        in_filename = file_list[j]
        img = Image.open(in_filename).convert("RGB")
        todraw = ([dict(name='True', Y=Yt, color=cf.truecolor)] if show_true else []) + \
                 [dict(name='Pred', Y=Yp, color=cf.predcolor)]
        csv_str = ''
        d = ImageDraw.Draw(img)
        for an in range(n_pred):
            for td in todraw:
                cx, cy, a, b, angle, noobj, rings = cleanup_antinode_vars(
                    td['Y'][j, an * cf.vars_per_pred:(an + 1) * cf.vars_per_pred])
                if noobj == 0 and rings > 0 and a >= 0 and b >= 0:
                    draw_ellipse(img, [cx, cy], [a, b], angle, color=td['color'], thickness=3)
                    d.text((cx - 10, cy - 8 + (0 if td['name'] == 'True' else 14)), "{: >3.1f}".format(rings),
                           fill=tuple(td['color'][::-1]))
                    if td['name'] == 'Pred' and out_csv is not None:
                        csv_str += "{},{},{},{},{},{},{}\n".format(cx, cy, os.path.basename(in_filename), rings, a, b, angle)
        if out_csv is not None and csv_str == '':
            csv_str = '0,0,' + os.path.basename(in_filename) + ',0,0,0,0\n'
        d.text((5, orig_img_dims[1] - 14), os.path.basename(in_filename), fill=(255, 255, 255))
        if png == "host":
            img.save(log_dir + '/steelpan_pred_' + str(j).zfill(5) + '.png')
        if sink.wants_device_frames:
            frame = np.asarray(img, dtype=np.uint8)
            if held and (held[0][0].shape != frame.shape or len(held) >= png_chunk):
                flush()
            held.append((frame, log_dir + '/steelpan_pred_' + str(j).zfill(5) + sink.extension))
        if out_csv is not None:
            with open(out_csv, "a") as f:
                f.write(csv_str)
    flush()


def _show_pred_ellipses_device(Yt, Yp, file_list, num_draw, log_dir, out_csv, show_true, png, png_chunk, device_decode,
                               sink, given=None):
    """show_pred_ellipses(draw="device"): runs of frames of one size, at most png_chunk long, are loaded, planned, drawn
    by csrc/overlay.hip and written; the CSV rows of a chunk are appended once its files are written."""
    import torch
    from . import overlay
    if not torch.cuda.is_available():
        raise RuntimeError('show_pred_ellipses: draw="device" draws on the GPU (no CPU fallback)')
    num_draw = min(num_draw, Yt.shape[0], len(file_list))
    if given is not None:
        num_draw = min(num_draw, int(given.shape[0]))
    if out_csv is not None:
        open(out_csv, "w").close()
    png_chunk = max(int(png_chunk), 1)

    def finish(lo, frames):
        """frames: uint8 device tensor [n,H,W] (grey) or [n,H,W,3] of files lo .. lo+n-1, one size."""
        n = int(frames.shape[0])
        plan = overlay.plan_overlays(Yt[lo:lo + n], Yp[lo:lo + n], file_list[lo:lo + n], show_true=show_true,
                                     size=tuple(int(v) for v in frames.shape[1:3]), with_csv=out_csv is not None)
        drawn = overlay.draw_overlays_device(frames, plan)
        paths = [log_dir + '/steelpan_pred_' + str(lo + k).zfill(5) + sink.extension for k in range(n)]
        sink.write(drawn, paths)
        if png == "host":
            host = drawn.cpu().numpy()
            for k in range(n):
                Image.fromarray(host[k]).save(paths[k])
        if out_csv is not None:
            with open(out_csv, "a") as f:
                f.write(''.join(plan.csv))

    def decode_on_device(names):
        """uint8 device frames [n,H,W] | [n,H,W,3] equal to Image.open(f).convert("RGB") of every file, or None where the
        device decoder does not give that for this chunk (mixed sizes or kinds, a palette or 16-bit file): Pillow then."""
        from .jpeg import read_frames_device
        try:
            frames, _, fallback = read_frames_device(names, channels="all", return_info=True)
        except ValueError:
            return None
        if fallback:
            return None
        c = int(frames.shape[3])                    # grey, grey + alpha, RGB, RGBA: convert("RGB") drops the alpha
        return frames[..., 0] if c <= 2 else frames[..., :3]

    for lo in range(0, num_draw, png_chunk):
        names = list(file_list[lo:min(lo + png_chunk, num_draw)])
        if given is not None:
            finish(lo, given[lo:lo + len(names)])
            continue
        frames = decode_on_device(names) if device_decode else None
        if frames is not None:
            finish(lo, frames)
            continue
        loaded = [np.asarray(Image.open(f).convert("RGB"), dtype=np.uint8) for f in names]
        k = 0
        while k < len(loaded):                      # runs of one size: frames of mixed size are chunked by size
            e = k + 1
            while e < len(loaded) and loaded[e].shape == loaded[k].shape:
                e += 1
            finish(lo + k, torch.from_numpy(np.stack(loaded[k:e])).cuda())
            k = e
