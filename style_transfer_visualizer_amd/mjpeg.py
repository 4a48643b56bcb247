"""Motion-JPEG timelapse video (``--video-format mjpeg``; the reference encodes H.264 through ffmpeg on the host, which this
build cannot reach).

Every saved frame becomes one baseline JPEG - 4:2:0, the Annex K Huffman tables of ITU T.81, libjpeg's quality scaling - and
the frames go into an AVI container (``MJPG``), which needs a few hundred bytes of RIFF headers and an index.  During the run
a saved frame costs two launches and no host synchronisation: ``ops.image_to_u8`` writes the reference's frame conversion
into one staging frame and ``ops.jpeg_dct`` turns it into quantised coefficients in the next slot of a store allocated before
the run.  When the run is over, ``ops.jpeg_block_bits`` and ``ops.jpeg_scan`` size and place every block's Huffman code,
``ops.jpeg_emit`` writes the codes, the streams cross to the host in batches, and the host adds what is serial and tiny:
``0xFF`` stuffing, the headers, the container.

Definitions, to the bit, are in ``include/stv.h``; ``tests/jpeg_ref.py`` holds NumPy twins of the kernels.
"""
from __future__ import annotations

import struct
import time
from pathlib import Path

import numpy as np
import torch

from .constants import IMAGENET_MEAN, IMAGENET_STD
from .logging_utils import logger

MJPEG_MAX_DEVICE_BYTES = 4 << 30        # the coefficient store: 3 bytes per padded pixel and frame
EMIT_BATCH_BYTES = 256 << 20            # streams written and copied per batch of frames
AVI_MAX_BYTES = (1 << 31) - (1 << 20)   # a plain (not OpenDML) AVI stays under 2 GiB
MAX_DIM = 65535                         # SOF0 holds the frame size in 16 bits
MAX_BLOCK_BITS = 1664                   # stv.h STV_JPEG_MAX_BLOCK_BITS: bit offsets inside a frame are 32 bits wide

# `--quality q` (1..10) -> libjpeg quality Q = min(95, 10*q + 5).  A design choice, not derived: q = 5 lands next to libjpeg's
# default of 75 scaled to this range, q = 10 at 95, past which files grow much faster than they improve.
QUALITY_TO_JPEG = {1: 15, 2: 25, 3: 35, 4: 45, 5: 55, 6: 65, 7: 75, 8: 85, 9: 95, 10: 95}

DEFAULT_TITLE = "Style Transfer Visualizer Output"      # the reference's default metadata strings
DEFAULT_ARTIST = "Style Transfer Visualizer"

# ITU T.81 Annex K.1: the two example quantisation tables, row-major (row v: vertical frequency)
LUMA_BASE = (
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99,
)
CHROMA_BASE = (
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
)

# ITU T.81 Annex K.3: the four "typical" Huffman tables as (BITS: codes of length 1..16, HUFFVAL)
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), (
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), (
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa))
# (class, table id) in the order the headers carry them: DC 0, AC 0, DC 1, AC 1
HUFFMAN_TABLES = ((0, 0, DC_LUMA), (1, 0, AC_LUMA), (0, 1, DC_CHROMA), (1, 1, AC_CHROMA))


def _zigzag() -> tuple[int, ...]:
    """``ZIGZAG[i]``: the row-major index ``v*8 + u`` of the coefficient at position ``i`` of the zigzag order."""
    order, v, u = [], 0, 0
    for _ in range(64):
        order.append(v * 8 + u)
        if (v + u) % 2 == 0:            # up and to the right
            if u == 7:                  # noqa: PLR2004
                v += 1
            elif v == 0:
                u += 1
            else:
                v, u = v - 1, u + 1
        elif v == 7:                    # noqa: PLR2004   (down and to the left)
            u += 1
        elif u == 0:
            v += 1
        else:
            v, u = v + 1, u - 1
    return tuple(order)


ZIGZAG = _zigzag()


def jpeg_quality(quality: int) -> int:
    """The libjpeg quality of ``--quality`` 1..10."""
    if quality not in QUALITY_TO_JPEG:
        msg = f"Video quality must be between 1 and 10, got {quality}"
        raise ValueError(msg)
    return QUALITY_TO_JPEG[quality]


def quant_tables(jpeg_q: int) -> np.ndarray:
    """The two quantisation tables at libjpeg quality ``jpeg_q`` (1..100), int32 ``[2, 64]`` row-major: the Annex K tables
    scaled by libjpeg's rule, ``s = 5000 // Q`` below 50 and ``200 - 2Q`` from there, ``(base*s + 50) // 100`` clamped to
    1..255 (baseline)."""
    jpeg_q = int(jpeg_q)
    if not 1 <= jpeg_q <= 100:          # noqa: PLR2004
        msg = f"JPEG quality must be between 1 and 100, got {jpeg_q}"
        raise ValueError(msg)
    scale = 5000 // jpeg_q if jpeg_q < 50 else 200 - 2 * jpeg_q      # noqa: PLR2004
    base = np.array([LUMA_BASE, CHROMA_BASE], dtype=np.int64)
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.int32)


def check_qtabs(qtabs) -> np.ndarray:
    q = np.asarray(qtabs)
    if q.size != 128 or int(q.min()) < 1 or int(q.max()) > 255:      # noqa: PLR2004
        msg = "quantisation tables: two tables of 64 entries in 1..255 are expected"
        raise ValueError(msg)
    return q.astype(np.int32).reshape(2, 64)


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def jpeg_headers(H: int, W: int, qtabs) -> bytes:
    """Everything of a frame's JFIF file in front of the scan: SOI, APP0 ``JFIF`` 1.01, two DQT, SOF0 (8 bit, three components,
    Y 2x2 on table 0, Cb and Cr 1x1 on table 1), four DHT, SOS.  The scan (stuffed) and EOI follow."""
    check_frame_size(H, W)
    q = check_qtabs(qtabs)
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\x00" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))]
    out += [_segment(0xDB, bytes([t]) + bytes(int(q[t][ZIGZAG[i]]) for i in range(64))) for t in range(2)]
    out.append(_segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    out += [_segment(0xC4, bytes([cls << 4 | tid]) + bytes(bits) + bytes(vals)) for cls, tid, (bits, vals) in HUFFMAN_TABLES]
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


EOI = b"\xff\xd9"


def stuff(scan: bytes) -> bytes:
    """Byte stuffing of an entropy-coded segment: a zero byte behind every ``0xFF``."""
    return bytes(scan).replace(b"\xff", b"\xff\x00")


def _chunk(fourcc: bytes, payload: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) % 2 else b"")


def _info_list(info: dict[str, str]) -> bytes:
    body = b"INFO"
    for fourcc, key in ((b"INAM", "title"), (b"IART", "artist"), (b"ISFT", "software")):
        if info.get(key):
            body += _chunk(fourcc, str(info[key]).encode("utf-8") + b"\x00")
    return _chunk(b"LIST", body)


def write_avi(path: str | Path, frames: list[bytes], W: int, H: int, fps: int, info: dict[str, str] | None = None) -> int:   # noqa: PLR0913
    """Write ``frames`` (complete JPEG files of ``W x H`` pixels) as a Motion-JPEG AVI at ``fps / 1`` frames per second:
    ``RIFF AVI`` = ``hdrl`` (``avih``, one ``strl`` of ``strh`` ``vids``/``MJPG`` and ``strf``, a BITMAPINFOHEADER) + ``LIST INFO``
    (``info``: title -> ``INAM``, artist -> ``IART``, software -> ``ISFT``) + ``LIST movi`` of ``00dc`` chunks padded to even
    length + ``idx1`` (offsets from the ``movi`` tag).  The file stays under ``AVI_MAX_BYTES``: frames that would not fit are
    left out, with one warning that names both counts (OpenDML is not built).  Returns the number of frames written."""
    fps = int(fps)
    if fps < 1:
        msg = f"fps must be at least 1, got {fps}"
        raise ValueError(msg)
    check_frame_size(H, W)
    info_list = _info_list(info or {})
    # RIFF header 12, hdrl list 12 + avih 64 + strl list 12 + strh 64 + strf 48, the movi list header 12, the idx1 header 8
    fixed = 12 + (12 + 64 + 12 + 64 + 48) + len(info_list) + 12 + 8
    kept, size = 0, fixed
    for frame in frames:
        need = 8 + len(frame) + len(frame) % 2 + 16
        if size + need > AVI_MAX_BYTES:
            break
        kept, size = kept + 1, size + need
    if kept < len(frames):
        logger.warning("MJPEG timelapse: %d of %d frames fit a plain AVI file of at most %d bytes; the file is closed after frame %d "
                       "(save fewer frames with a larger --save-every, or lower --quality)", kept, len(frames), AVI_MAX_BYTES, kept)
    frames = frames[:kept]
    largest = max((len(f) for f in frames), default=0)
    total = sum(len(f) for f in frames)
    avih = struct.pack("<14I", 1000000 // fps, (total * fps) // max(kept, 1), 0, 0x10, kept, 0, 1, largest, W, H, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, 1, fps, 0, kept, largest, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    strl = _chunk(b"LIST", b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf))
    hdrl = _chunk(b"LIST", b"hdrl" + _chunk(b"avih", avih) + strl)
    movi, index, at = [b"movi"], [], 4
    for frame in frames:
        index.append(b"00dc" + struct.pack("<III", 0x10, at, len(frame)))
        piece = _chunk(b"00dc", frame)
        movi.append(piece)
        at += len(piece)
    body = b"AVI " + hdrl + info_list + _chunk(b"LIST", b"".join(movi)) + _chunk(b"idx1", b"".join(index))
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    with path.open("wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", len(body)))
        fh.write(body)
    return kept


def check_frame_size(H: int, W: int) -> None:
    """Refuse a frame a baseline JPEG cannot describe, or whose bit offsets would not fit 32 bits."""
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H > MAX_DIM or W > MAX_DIM:
        msg = f"the MJPEG timelapse takes frames of 1 to {MAX_DIM} pixels a side (a JPEG stores its size in 16 bits), got {W}x{H}"
        raise ValueError(msg)
    blocks = padded_pixels(H, W) // 256 * 6
    if blocks * MAX_BLOCK_BITS >= 1 << 32:
        msg = (f"the MJPEG timelapse addresses a frame's code with 32-bit bit offsets: {W}x{H} pixels are {blocks} blocks of up to "
               f"{MAX_BLOCK_BITS} bits, over 2^32")
        raise ValueError(msg)


def padded_pixels(H: int, W: int) -> int:
    """Pixels of a frame padded to whole 16x16 MCUs."""
    return ((int(H) + 15) // 16) * ((int(W) + 15) // 16) * 256


def store_bytes(n_frames: int, H: int, W: int) -> int:
    """Device bytes of the coefficient store of ``n_frames`` frames of ``H x W`` pixels: int16 for every sample of the padded
    4:2:0 frame, 3 bytes per padded pixel."""
    return int(n_frames) * padded_pixels(H, W) * 3


def check_budget(n_frames: int, H: int, W: int) -> int:
    """Refuse a timelapse whose coefficients do not fit ``MJPEG_MAX_DEVICE_BYTES`` (spilling to the host is not built)."""
    need = store_bytes(n_frames, H, W)
    if need > MJPEG_MAX_DEVICE_BYTES:
        msg = (f"the MJPEG timelapse keeps its frames on the device: {n_frames} frames of {W}x{H} pixels need {need} bytes, over the "
               f"budget of {MJPEG_MAX_DEVICE_BYTES} bytes; save fewer frames with a larger --save-every")
        raise ValueError(msg)
    return need


def video_info(title: str | None, artist: str | None) -> dict[str, str]:
    """The strings of the ``LIST INFO`` chunk: the reference's defaults where none is given."""
    from .runtime.version import resolve_project_version  # noqa: PLC0415
    return {"title": title or DEFAULT_TITLE, "artist": artist or DEFAULT_ARTIST,
            "software": f"style_transfer_visualizer_amd v{resolve_project_version()}"}


class DeviceMjpegWriter:
    """A ``FrameSink`` that keeps quantised DCT coefficients on the device and writes one Motion-JPEG AVI on ``close()``.

    Everything the run needs is allocated here: one staging frame ``[H, W, 3]`` uint8 (reused for every frame: the launches
    of one frame are in stream order in front of the next frame's), the coefficient store int16 ``[n_frames, blocks, 64]``, and
    the length, offset and total arrays.  ``append_device`` enqueues two launches on the current stream and returns: no
    synchronisation, no device allocation, no host read.  ``close()`` codes the frames and writes the file."""

    def __init__(self, path: str | Path, fps: int, H: int, W: int, n_frames: int, *, quality: int = 10,  # noqa: PLR0913
                 info: dict[str, str] | None = None, device: torch.device | str = "cuda") -> None:
        from . import ops  # noqa: PLC0415
        self.path = Path(path)
        self.H, self.W, self.n_frames, self.fps = int(H), int(W), int(n_frames), int(fps)
        if self.n_frames < 0 or self.fps < 1:
            msg = f"DeviceMjpegWriter: {self.n_frames} frames at {self.fps} frames per second"
            raise ValueError(msg)
        check_frame_size(self.H, self.W)
        self.jpeg_quality = jpeg_quality(quality)
        self.qtabs = quant_tables(self.jpeg_quality)
        check_budget(self.n_frames, self.H, self.W)             # before anything is allocated or launched
        self.info = dict(info) if info is not None else video_info(None, None)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            msg = f"DeviceMjpegWriter keeps its frames on a GPU, got device {self.device}"
            raise RuntimeError(msg)
        self.blocks = ops.jpeg_blocks(self.H, self.W)
        self.count = 0
        self.closed = False
        self.frames_written = 0
        self.file_bytes = 0
        self.timings: dict[str, float] = {}
        self._staging = self._coef = self._bits = self._offsets = self._totals = None
        if self.n_frames:
            self._staging = torch.empty(self.H, self.W, 3, dtype=torch.uint8, device=self.device)
            self._coef = torch.empty(self.n_frames, self.blocks, 64, dtype=torch.int16, device=self.device)
            self._bits = torch.empty(self.n_frames, self.blocks, dtype=torch.int32, device=self.device)
            self._offsets = torch.empty(self.n_frames, self.blocks, dtype=torch.int32, device=self.device)
            self._totals = torch.empty(self.n_frames, dtype=torch.int32, device=self.device)

    def _next_slot(self) -> torch.Tensor:
        if self.closed:
            msg = "DeviceMjpegWriter: a frame appended after close()"
            raise RuntimeError(msg)
        if self.count >= self.n_frames:
            msg = f"DeviceMjpegWriter: frame {self.count + 1} appended to a store of {self.n_frames} frames"
            raise RuntimeError(msg)
        return self._coef[self.count]

    def append_device(self, image: torch.Tensor, *, normalize: bool) -> None:
        """Capture the image being optimised (fp32 ``[1, 3, H, W]`` or ``[3, H, W]`` on the device) as the next frame."""
        from . import ops  # noqa: PLC0415
        if tuple(image.shape[-2:]) != (self.H, self.W):
            msg = f"DeviceMjpegWriter: a frame of {tuple(image.shape[-2:])} for a store of {(self.H, self.W)}"
            raise RuntimeError(msg)
        slot = self._next_slot()
        ops.image_to_u8(image, mean=IMAGENET_MEAN if normalize else None, std=IMAGENET_STD if normalize else None,
                        rounding=False, out=self._staging)
        ops.jpeg_dct(self._staging, self.qtabs, out=slot)
        self.count += 1

    def append_data(self, frame: np.ndarray) -> None:
        """The ``FrameSink`` protocol: a host frame, uint8 ``[H, W, 3]``, is uploaded into the staging frame."""
        from . import ops  # noqa: PLC0415
        arr = np.ascontiguousarray(frame)
        if arr.dtype != np.uint8 or arr.shape != (self.H, self.W, 3):
            msg = f"DeviceMjpegWriter: a host frame of {arr.shape} {arr.dtype} for a store of {(self.H, self.W, 3)} uint8"
            raise RuntimeError(msg)
        slot = self._next_slot()
        self._staging.copy_(torch.from_numpy(arr))
        ops.jpeg_dct(self._staging, self.qtabs, out=slot)
        self.count += 1

    def close(self) -> None:
        """Write the file (once; further calls do nothing) and free the store."""
        if self.closed:
            return
        self.closed = True
        try:
            if self.count == 0:
                logger.info("MJPEG timelapse: no frame was saved, %s is not written", self.path)
                return
            self._encode()
        finally:
            self._staging = self._coef = self._bits = self._offsets = self._totals = None

    def _encode(self) -> None:
        from . import ops  # noqa: PLC0415
        clock = time.perf_counter
        n = self.count
        t0 = clock()
        coef, bits, offsets, totals = self._coef[:n], self._bits[:n], self._offsets[:n], self._totals[:n]
        ops.jpeg_block_bits(coef, out=bits)
        ops.jpeg_scan(bits, offsets, totals)
        total_bits = totals.cpu().numpy().view(np.uint32).astype(np.int64)
        t1 = clock()
        nbytes = (total_bits + 7) // 8
        region = (nbytes + 3) // 4 * 4                       # a frame's stream starts on a 32-bit word
        header = jpeg_headers(self.H, self.W, self.qtabs)
        files: list[bytes] = []
        emit_s = copy_s = stuff_s = 0.0
        first = 0
        while first < n:
            last, size = first + 1, int(region[first])       # (a batch holds at least one frame)
            while last < n and size + int(region[last]) <= EMIT_BATCH_BYTES:
                size += int(region[last])
                last += 1
            ta = clock()
            base = np.concatenate([[0], np.cumsum(region[first:last])[:-1]]).astype(np.int32)
            stream = torch.zeros(size, dtype=torch.uint8, device=self.device)
            ops.jpeg_emit(coef[first:last], offsets[first:last], torch.from_numpy(base).to(self.device), stream)
            torch.cuda.synchronize(self.device)
            tb = clock()
            host = stream.cpu().numpy()
            tc = clock()
            for i in range(first, last):
                at = int(base[i - first])
                files.append(header + stuff(host[at:at + int(nbytes[i])].tobytes()) + EOI)
            td = clock()
            emit_s, copy_s, stuff_s = emit_s + (tb - ta), copy_s + (tc - tb), stuff_s + (td - tc)
            del stream
            first = last
        t2 = clock()
        self.frames_written = write_avi(self.path, files, self.W, self.H, self.fps, self.info)
        t3 = clock()
        self.file_bytes = self.path.stat().st_size
        self.timings = {"bits_scan_s": t1 - t0, "emit_s": emit_s, "copy_s": copy_s, "stuff_s": stuff_s, "avi_s": t3 - t2}
        logger.info("MJPEG timelapse: %d frames, JPEG quality %d, %d frames per second, %d bytes", self.frames_written,
                    self.jpeg_quality, self.fps, self.file_bytes)
