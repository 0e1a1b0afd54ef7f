"""Frame preprocessing on libsola_hip.so: PIL's 8-bit resize, byte for byte, and the normalisation behind it.

What SAM2's video predictor does to every frame on the host before its first kernel runs (``init_state`` ->
``load_video_frames``: ``Image.open(p).convert("RGB").resize((S, S))``, ``/ 255.0``, ``-= mean``, ``/= std``) and what
GroundingDINO's transform does to its image (``RandomResize([800], max_size=1333)``, ``ToTensor``, ``Normalize``), from uint8
frames on the device.  JPEG decode stays on the host by default; ``decode_jpeg`` and ``load_video_frames(jpeg_decoder="gpu")``
decode baseline files on the device, the bytes of ``Image.open(f).convert("RGB")``.  Upstream details are quoted from the public
sources; no end-to-end run with either model was made.

A byte has 256 values, so a normalisation recipe is a float32 ``[C,256]`` table, built on the host with the recipe's own torch
and numpy operations (``normalise_table``): the floats are the recipe's, not a restatement of it."""
from __future__ import annotations

import ctypes as C
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ._lib import SolaError, check, current_stream, lib, ptr, require_cuda
from .seg_utils import _stream_scratch

FILTERS = {"bilinear": 2, "bicubic": 3}  # PIL.Image.Resampling's numbers = SOLA_RESAMPLE_*
MAX_SIZE = 16384
TILE_W = TILE_H = 64           # SOLA_RESAMPLE_TILE_*: output pixels a block owns
READER_THREADS = 8             # JPEG decode threads of load_video_frames (a constant: never the machine's CPU count)
CHUNK_FRAMES = 16              # frames decoded, uploaded and preprocessed at a time
SAM2_MEAN, SAM2_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

JPEG_DECODERS = ("pil", "gpu")
JPEG_SUBSEQ_MIN, JPEG_SUBSEQ_DEFAULT = 16, 128   # SOLA_JPEG_SUBSEQ_MIN / _DEFAULT

_TABLES = {}
_TABLES_LOCK = threading.Lock()


def _filter_id(filter):
    try:
        return FILTERS[filter]
    except (KeyError, TypeError):
        raise SolaError(f"filter {filter!r}: 'bilinear' or 'bicubic'") from None


def resample_coeffs(in_size, out_size, filter="bicubic"):
    """(bounds int32 [out,2], coeffs int32 [out,taps]) of one axis on the host: sola_resample_coeffs, Pillow's precompute_coeffs and
    normalize_coeffs_8bpc."""
    f = _filter_id(filter)
    taps = lib().sola_resample_taps(int(in_size), int(out_size), f)
    check(0 if taps > 0 else -1, "sola_resample_taps")
    bounds = np.empty((out_size, 2), np.int32)
    coeffs = np.empty((out_size, taps), np.int32)
    check(lib().sola_resample_coeffs(int(in_size), int(out_size), f, C.c_void_p(bounds.ctypes.data), C.c_void_p(coeffs.ctypes.data)),
          "sola_resample_coeffs")
    return bounds, coeffs


def _axis_table(in_size, out_size, filter, device):
    """The device table int32 [out, 2 + taps] of an axis and its taps, cached by (in, out, filter, device); (None, 0) for an axis
    that keeps its size (Pillow skips that pass)."""
    if in_size == out_size:
        return None, 0
    key = (int(in_size), int(out_size), filter, str(device))
    with _TABLES_LOCK:
        hit = _TABLES.get(key)
    if hit is None:
        bounds, coeffs = resample_coeffs(in_size, out_size, filter)
        hit = (torch.from_numpy(np.concatenate([bounds, coeffs], axis=1)).to(device), coeffs.shape[1])
        with _TABLES_LOCK:
            _TABLES[key] = hit
    return hit


def _frames(images):
    require_cuda(images)
    if images.dtype != torch.uint8 or images.dim() not in (3, 4) or images.shape[-1] not in (1, 3):
        raise SolaError(f"frames must be uint8 [T,H,W,C] or [H,W,C] with C 1 or 3, got {images.dtype} {tuple(images.shape)}")
    return images.contiguous() if images.dim() == 4 else images.contiguous()[None]


def _size(size):
    h, w = (int(v) for v in size)
    return h, w


@torch.no_grad()
def _resample(src, size, filter, table, out=None):
    T, H, W, Cn = src.shape
    h, w = _size(size)
    dev = src.device
    _filter_id(filter)
    for n in (H, W, h, w):
        if not 1 <= n <= MAX_SIZE:
            raise SolaError(f"resample: axis of {n} pixels, 1 .. {MAX_SIZE} are supported")
    tx, taps_x = _axis_table(W, w, filter, dev)
    ty, taps_y = _axis_table(H, h, filter, dev)
    if table is None:
        shape, dtype = (T, h, w, Cn), torch.uint8
    else:
        if table.dtype != torch.float32 or tuple(table.shape) != (Cn, 256):
            raise SolaError(f"normalisation table must be float32 [{Cn},256], got {table.dtype} {tuple(table.shape)}")
        table = table.to(dev).contiguous()
        shape, dtype = (T, Cn, h, w), torch.float32
    if out is None:
        out = torch.empty(shape, device=dev, dtype=dtype)
    elif out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
        raise SolaError(f"resample: out must be a contiguous {dtype} {shape} on {dev}")
    need = lib().sola_resample_u8_scratch_bytes(T, H, W, Cn, h, w, taps_x, taps_y)
    scratch = _stream_scratch("resample", dev, need) if need else None
    check(lib().sola_resample_u8(ptr(src), T, H, W, Cn, h, w, ptr(tx), taps_x, ptr(ty), taps_y, ptr(table), ptr(out), ptr(scratch), need,
                                 current_stream(dev)), "sola_resample_u8")
    return out


def resize_u8(images, size, filter="bicubic"):
    """uint8 ``[T,H,W,C]`` or ``[H,W,C]`` on the GPU -> uint8 of the same rank with ``size = (h, w)``: the bytes of
    ``PIL.Image.resize(size[::-1], BICUBIC | BILINEAR)`` frame by frame (C = 1: mode "L", C = 3: "RGB")."""
    src = _frames(images)
    out = _resample(src, size, filter, None)
    return out if images.dim() == 4 else out[0]


def normalise_table(mean, std, recipe="sam2_video"):
    """The float32 ``[C,256]`` table ``byte -> normalised value`` of a recipe, made on the host by the recipe's own operations.
    ``"sam2_video"``: sam2/utils/misc.py's ``img_np / 255.0`` (numpy, float64), assigned into a float32 tensor, then the in-place
    ``-= mean`` and ``/= std``.  ``"to_tensor"``: torchvision's ``ToTensor`` (``.to(float32).div(255)``) and ``Normalize``
    (``.sub_(mean).div_(std)``)."""
    mean = torch.tensor([float(v) for v in mean], dtype=torch.float32)[:, None]
    std = torch.tensor([float(v) for v in std], dtype=torch.float32)[:, None]
    if mean.shape != std.shape or mean.shape[0] not in (1, 3):
        raise SolaError(f"mean and std must both have 1 or 3 entries, got {mean.shape[0]} and {std.shape[0]}")
    n = mean.shape[0]
    if recipe == "sam2_video":
        table = torch.zeros(n, 256, dtype=torch.float32)
        table[:] = torch.from_numpy(np.arange(256, dtype=np.uint8) / 255.0)
        table -= mean
        table /= std
    elif recipe == "to_tensor":
        table = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)[None].repeat(n, 1)
        table.sub_(mean).div_(std)
    else:
        raise SolaError(f"unknown recipe {recipe!r}: 'sam2_video' or 'to_tensor'")
    return table


def preprocess(images, size, filter, table, out=None):
    """uint8 ``[T,H,W,C]`` (or ``[H,W,C]``) on the GPU -> float32 ``[T,C,h,w]``: ``table[c][byte]`` of the PIL-exact resize, in
    one call.  ``table``: normalise_table's, on either side (a host table is uploaded)."""
    if table is None:
        raise SolaError("preprocess needs a normalisation table (normalise_table); resize_u8 returns the bytes")
    return _resample(_frames(images), size, filter, table, out)


# ------------------------------------------------------------------------------------------------------------- JPEG decode
class SolaJpegHuff(C.Structure):
    _fields_ = [("look", C.c_uint16 * 256), ("limit", C.c_uint32 * 18), ("valoff", C.c_int32 * 18), ("vals", C.c_uint8 * 256)]


class SolaJpegPlan(C.Structure):
    """include/sola_hip.h: what sola_jpeg_parse knows about one file."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32),
                ("mcus_x", C.c_int32), ("mcus_y", C.c_int32), ("blocks_per_mcu", C.c_int32), ("n_blocks", C.c_int32),
                ("restart_interval", C.c_int32), ("n_segments", C.c_int32), ("reserved", C.c_int32),
                ("scan_begin", C.c_int64), ("scan_end", C.c_int64), ("scan_offset", C.c_int64), ("seg_offset", C.c_int64),
                ("quant", (C.c_uint16 * 64) * 3), ("huff", SolaJpegHuff * 6)]


def _jpeg_bytes(f):
    if isinstance(f, (bytes, bytearray, memoryview)):
        return bytes(f)
    with open(f, "rb") as fh:
        return fh.read()


def jpeg_parse(data):
    """(SolaJpegPlan, segments int32 [n_segments, 2]) of one file's bytes (sola_jpeg_parse: host only); SolaError with the parser's
    reason for a file the GPU decoder does not take."""
    data = bytes(data)
    plan = SolaJpegPlan()
    segs = np.empty((64, 2), np.int32)
    for _ in range(2):
        check(lib().sola_jpeg_parse(data, len(data), C.byref(plan), C.c_void_p(segs.ctypes.data), segs.shape[0]), "sola_jpeg_parse")
        if plan.n_segments <= segs.shape[0]:
            break
        segs = np.empty((plan.n_segments, 2), np.int32)
    return plan, segs[:plan.n_segments]


def jpeg_info(data):
    """``{"size": (W, H), "mode": "L" | "RGB", "sampling": "grey" | "4:4:4" | "4:2:2" | "4:2:0", "restart_interval": MCUs}`` of a
    file's bytes, or SolaError with the reason why ``decode_jpeg`` refuses it (progressive, CMYK, ...)."""
    plan, _ = jpeg_parse(data)
    sampling = "grey" if plan.ncomp == 1 else {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0"}[(plan.hs, plan.vs)]
    return {"size": (plan.width, plan.height), "mode": "L" if plan.ncomp == 1 else "RGB", "sampling": sampling,
            "restart_interval": plan.restart_interval}


class _JpegChunk:
    """The host side of one sola_jpeg_decode call: plans with their offsets set, and ONE pinned blob [plans | segments | scans]."""

    def __init__(self, parsed, datas):
        self.T = len(parsed)
        self.plans = (SolaJpegPlan * self.T)()
        plan_bytes = C.sizeof(SolaJpegPlan) * self.T
        n_segs = sum(p.n_segments for p, _ in parsed)
        self.off_segs = plan_bytes
        off = self.off_scan = (plan_bytes + 8 * n_segs + 15) // 16 * 16
        seg_row = 0
        for t, (p, _) in enumerate(parsed):
            C.memmove(C.byref(self.plans[t]), C.byref(p), C.sizeof(SolaJpegPlan))
            self.plans[t].scan_offset, self.plans[t].seg_offset = off - self.off_scan, seg_row
            seg_row += p.n_segments
            off += (p.scan_end - p.scan_begin + 15) // 16 * 16
        self.n_segs, self.scan_bytes = n_segs, off - self.off_scan
        self.blob = torch.empty(max(off, 16), dtype=torch.uint8, pin_memory=True)
        host = self.blob.numpy()
        host[:plan_bytes] = np.frombuffer(self.plans, np.uint8)
        if n_segs:
            host[self.off_segs:self.off_segs + 8 * n_segs] = np.concatenate([s for _, s in parsed]).reshape(-1).view(np.uint8)
        for t, ((p, _), d) in enumerate(zip(parsed, datas)):
            o = self.off_scan + self.plans[t].scan_offset
            host[o:o + p.scan_end - p.scan_begin] = np.frombuffer(d, np.uint8, p.scan_end - p.scan_begin, p.scan_begin)


def _jpeg_geometry(p):
    return (p.width, p.height, p.ncomp, p.hs, p.vs)


@torch.no_grad()
def _jpeg_decode_chunk(parsed, datas, dev, subseq_bytes, out=None, want=None):
    """One sola_jpeg_decode call on frames of one geometry -> (uint8 [T,H,W,3] on dev, error words, sync rounds)."""
    chunk = _JpegChunk(parsed, datas)
    T, p0 = chunk.T, parsed[0][0]
    blob = chunk.blob.to(dev, non_blocking=True)
    if out is None:
        out = torch.empty((T, p0.height, p0.width, 3), dtype=torch.uint8, device=dev)
    need = lib().sola_jpeg_scratch_bytes(chunk.plans, T, int(subseq_bytes))
    check(0 if need else -1, "sola_jpeg_scratch_bytes")
    scratch = _stream_scratch("jpeg", dev, need)
    err = (C.c_int32 * T)()
    rounds = C.c_int32()
    base = blob.data_ptr()
    check(lib().sola_jpeg_decode(C.c_void_p(base + chunk.off_scan), chunk.scan_bytes, C.c_void_p(base + chunk.off_segs), chunk.n_segs, chunk.plans,
                                 C.c_void_p(base), T, int(subseq_bytes), ptr(out), ptr(scratch), need, err, C.byref(rounds), current_stream(dev)),
          "sola_jpeg_decode")
    if want is not None:  # tests: the coefficient buffer of frame `want`
        coef = np.empty((p0.n_blocks, 64), np.int16)
        check(lib().sola_jpeg_coefficients(chunk.plans, T, int(subseq_bytes), ptr(scratch), int(want), C.c_void_p(coef.ctypes.data), current_stream(dev)),
              "sola_jpeg_coefficients")
        return out, list(err), rounds.value, coef
    return out, list(err), rounds.value


def decode_jpeg(files, device=None, subseq_bytes=0, return_errors=False):
    """A list of baseline JPEG files (``bytes`` or paths) of one size and sampling -> uint8 ``[T,H,W,3]`` on the device: the bytes
    of ``Image.open(f).convert("RGB")`` frame by frame, entropy decode included on the GPU (sola_jpeg_decode; include/sola_hip.h
    has the supported files and the refusals).  ``subseq_bytes``: bytes of the scan one thread decodes, 0 = the default, else a power of
    two from JPEG_SUBSEQ_MIN on.  A file the parser refuses raises SolaError with its reason; so does a frame whose scan turns out
    damaged (its error word is not 0) unless ``return_errors`` - then ``(frames, [error word per frame])`` comes back and a damaged
    frame holds whatever its readable part decodes to."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise SolaError(f"sola_amd runs on the GPU only (device {dev}); there is no CPU fallback")
    datas = [_jpeg_bytes(f) for f in files]
    if not datas:
        raise SolaError("decode_jpeg: no files")
    parsed = [jpeg_parse(d) for d in datas]
    for t, (p, _) in enumerate(parsed):
        if _jpeg_geometry(p) != _jpeg_geometry(parsed[0][0]):
            raise SolaError(f"decode_jpeg: frame {t} {_jpeg_geometry(p)} differs from frame 0 {_jpeg_geometry(parsed[0][0])} "
                            "(width, height, components, luma sampling)")
    with torch.cuda.device(dev):
        out, err, _ = _jpeg_decode_chunk(parsed, datas, dev, subseq_bytes)
    if return_errors:
        return out, err
    if any(err):
        raise SolaError(f"decode_jpeg: damaged scan, error words {err} (include/sola_hip.h: sola_jpeg_decode)")
    return out


# ----------------------------------------------------------------------------------------------------------- SAM2 video frames
_JPEG_EXT = (".jpg", ".jpeg", ".JPG", ".JPEG")


def _decode_into(path, dst, size_wh):
    from PIL import Image
    with Image.open(path) as im:
        if im.size != size_wh:
            raise SolaError(f"{path}: frame of {im.size[0]}x{im.size[1]} in a video of {size_wh[0]}x{size_wh[1]}")
        dst.numpy()[...] = np.asarray(im.convert("RGB"))


def _read_or_decode(path, dst, size_wh):
    """The "gpu" mode's reader: the file's bytes and their plan, or - for a file the parser refuses - None after the PIL reader has
    decoded it into dst."""
    data = _jpeg_bytes(path)
    try:
        plan, segs = jpeg_parse(data)
    except SolaError:
        _decode_into(path, dst, size_wh)
        return None
    if (plan.width, plan.height) != size_wh:
        raise SolaError(f"{path}: frame of {plan.width}x{plan.height} in a video of {size_wh[0]}x{size_wh[1]}")
    return (plan, segs), data


def _upload_gpu_decoded(jobs, buf, n, dev):
    """A chunk of the "gpu" mode -> uint8 [n,H,W,3] on dev: frames the parser took are decoded there, one sola_jpeg_decode call per
    geometry (a video has one); the others are uploaded from the pinned buffer the PIL reader filled."""
    frames = None
    if any(j is None for j in jobs):  # (rare: the whole pinned chunk goes up, the decoded frames are written over their slots)
        frames = buf[:n].to(dev, non_blocking=True)
    groups = {}
    for j in range(n):
        if jobs[j] is not None:
            groups.setdefault(_jpeg_geometry(jobs[j][0][0]), []).append(j)
    for members in groups.values():
        out, err, _ = _jpeg_decode_chunk([jobs[j][0] for j in members], [jobs[j][1] for j in members], dev, 0)
        if any(err):
            raise SolaError(f"load_video_frames: damaged JPEG scan in a frame of the chunk (error words {err})")
        if len(members) == n:
            return out
        if frames is None:
            frames = torch.empty((n,) + tuple(buf.shape[1:]), dtype=torch.uint8, device=dev)
        frames[torch.tensor(members, device=dev)] = out
    return frames


def load_video_frames(video_path, image_size, offload_video_to_cpu, img_mean=SAM2_MEAN, img_std=SAM2_STD, async_loading_frames=False,
                      compute_device=None, jpeg_decoder="pil"):
    """Stand-in for ``sam2.utils.misc.load_video_frames``, the function ``SAM2VideoPredictor.init_state`` calls: a directory of
    ``<int>.jpg`` / ``.jpeg`` frames -> ``(images float32 [T,3,S,S], video_height, video_width)``, the same floats.  PIL decodes on
    the host in READER_THREADS threads into pinned uint8 buffers; CHUNK_FRAMES frames at a time are uploaded, resized (bicubic)
    and normalised on ``compute_device``.  ``offload_video_to_cpu=True`` hands the result back on the host.
    ``jpeg_decoder="gpu"``: the reader threads read the files' bytes and parse them on the host (sola_jpeg_parse), and one
    sola_jpeg_decode call per chunk decodes them on the device instead of PIL - the same bytes, hence the same floats.  A frame the
    parser refuses (progressive, CMYK, ...: include/sola_hip.h) is decoded by the PIL reader, that frame alone; the result is the
    same bytes either way.  The default ``"pil"`` is the path described first."""
    from PIL import Image
    if jpeg_decoder not in JPEG_DECODERS:
        raise SolaError(f"load_video_frames: jpeg_decoder {jpeg_decoder!r}: one of {JPEG_DECODERS}")
    if async_loading_frames:
        raise SolaError("load_video_frames: async_loading_frames is not supported (frames are loaded in chunks by reader threads)")
    if not isinstance(video_path, (str, os.PathLike)) or not os.path.isdir(video_path):
        raise SolaError(f"load_video_frames: {video_path!r} is not a directory of JPEG frames (video files are not decoded here)")
    names = [p for p in os.listdir(video_path) if os.path.splitext(p)[-1] in _JPEG_EXT]
    try:
        names.sort(key=lambda p: int(os.path.splitext(p)[0]))
    except ValueError:
        raise SolaError(f"load_video_frames: frame names in {video_path} must be <int>.jpg") from None
    if not names:
        raise SolaError(f"load_video_frames: no JPEG frames in {video_path}")
    dev = torch.device("cuda", torch.cuda.current_device()) if compute_device is None else torch.device(compute_device)
    if dev.type != "cuda":
        raise SolaError(f"sola_amd runs on the GPU only (compute_device {dev}); there is no CPU fallback")
    paths = [os.path.join(video_path, n) for n in names]
    with Image.open(paths[0]) as im:
        W, H = im.size
    S, T = int(image_size), len(paths)
    table = normalise_table(img_mean, img_std, "sam2_video").to(dev)
    images = torch.empty((T, 3, S, S), dtype=torch.float32, device="cpu" if offload_video_to_cpu else dev,
                         pin_memory=bool(offload_video_to_cpu))
    n_chunk = min(CHUNK_FRAMES, T)
    pinned = [torch.empty((n_chunk, H, W, 3), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    ready = [None, None]  # the event after which a pinned buffer may be overwritten
    with torch.cuda.device(dev), ThreadPoolExecutor(max_workers=READER_THREADS) as pool:
        for ci, lo in enumerate(range(0, T, n_chunk)):
            n = min(n_chunk, T - lo)
            buf = pinned[ci & 1]
            if ready[ci & 1] is not None:
                ready[ci & 1].synchronize()
            if jpeg_decoder == "gpu":
                jobs = list(pool.map(lambda j: _read_or_decode(paths[lo + j], buf[j], (W, H)), range(n)))
                frames = _upload_gpu_decoded(jobs, buf, n, dev)
            else:
                list(pool.map(lambda j: _decode_into(paths[lo + j], buf[j], (W, H)), range(n)))  # (re-raises a reader's error)
                frames = buf[:n].to(dev, non_blocking=True)
            ready[ci & 1] = torch.cuda.Event()
            ready[ci & 1].record()
            if offload_video_to_cpu:
                images[lo:lo + n].copy_(preprocess(frames, (S, S), "bicubic", table), non_blocking=True)
            else:
                preprocess(frames, (S, S), "bicubic", table, out=images[lo:lo + n])
        torch.cuda.current_stream(dev).synchronize()
    return images, H, W


# ------------------------------------------------------------------------------------------------------------ GroundingDINO
def gdino_size(w, h, short=800, max_size=1333):
    """(w, h) after GroundingDINO's ``RandomResize([short], max_size)`` (datasets/transforms.py get_size_with_aspect_ratio)."""
    w, h, size = int(w), int(h), int(short)
    if max_size is not None:
        lo, hi = float(min(w, h)), float(max(w, h))
        if hi / lo * size > max_size:
            size = int(round(max_size * lo / hi))
    if (w <= h and w == size) or (h <= w and h == size):
        return w, h
    if w < h:
        return size, int(size * h / w)
    return int(size * w / h), size


def gdino_image(image, short=800, max_size=1333, mean=SAM2_MEAN, std=SAM2_STD, device=None):
    """GroundingDINO's ``transform_gd`` (RandomResize([short], max_size), ToTensor, Normalize) -> float32 ``[3,h,w]`` on the
    device.  ``image``: a PIL image (converted to RGB and uploaded) or uint8 ``[H,W,3]`` on the GPU."""
    if isinstance(image, torch.Tensor):
        require_cuda(image)
        src = image
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        src = torch.from_numpy(np.array(image.convert("RGB"))).to(dev)
    if src.dtype != torch.uint8 or src.dim() != 3 or src.shape[-1] != 3:
        raise SolaError(f"gdino_image: uint8 [H,W,3] or a PIL image, got {src.dtype} {tuple(src.shape)}")
    H, W = src.shape[:2]
    w, h = gdino_size(W, H, short, max_size)
    return preprocess(src, (h, w), "bilinear", normalise_table(mean, std, "to_tensor"))[0]
