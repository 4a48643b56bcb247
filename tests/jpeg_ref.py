"""NumPy twins of the four JPEG kernels (``style_transfer_visualizer_amd/csrc/jpeg.hip``), written from the definitions in
``include/stv.h``, and a small RIFF reader for the container tests.

* ``dct_quant(frame, qtabs)``: colour conversion, 4:2:0 chroma, level shift, the fixed-point DCT and the quantisation -
  ``stv_jpeg_dct``, int16 ``[blocks, 64]`` in zigzag order.  ``dct_stages`` exposes the intermediate values of the two passes.
* ``block_bits(coefs)``: the code length of every block of one frame - ``stv_jpeg_block_bits``.
* ``encode_scan(coefs)``: the entropy-coded segment of one frame before byte stuffing, padded with 1-bits - what
  ``stv_jpeg_scan`` and ``stv_jpeg_emit`` leave in a frame's stream.
The Huffman codes are derived here from the BITS / HUFFVAL lists of ``mjpeg.py`` (checked against PIL's in the host tests).
"""
from __future__ import annotations

import struct

import numpy as np

from style_transfer_visualizer_amd import _lib, mjpeg

T = np.array(_lib.JPEG_DCT_TABLE, dtype=np.int64)            # T[u][x]


def pad_frame(frame: np.ndarray) -> np.ndarray:
    """The frame extended to whole 16x16 MCUs by replicating its last column and row, int64."""
    H, W, _ = frame.shape
    ys = np.minimum(np.arange((H + 15) // 16 * 16), H - 1)
    xs = np.minimum(np.arange((W + 15) // 16 * 16), W - 1)
    return frame[ys][:, xs].astype(np.int64)


def samples(frame: np.ndarray) -> np.ndarray:
    """Level-shifted 8x8 sample blocks ``[blocks, 8, 8]`` in scan order: per MCU Y00 Y01 Y10 Y11 Cb Cr."""
    p = pad_frame(frame)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16
    assert Y.min() >= 0 and Y.max() <= 255 and Cb.min() >= 0 and Cb.max() <= 255 and Cr.min() >= 0 and Cr.max() <= 255
    mh, mw = p.shape[0] // 16, p.shape[1] // 16

    def down(c):
        return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    yb = (Y - 128).reshape(mh, 2, 8, mw, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mh, mw, 4, 8, 8)
    cb = (down(Cb) - 128).reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3)[:, :, None]
    cr = (down(Cr) - 128).reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3)[:, :, None]
    return np.concatenate([yb, cb, cr], axis=2).reshape(-1, 8, 8)


def dct_stages(s: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(a, a1, b)`` of sample blocks ``[n, 8(y), 8(x)]``: the row sums, their rounded shift, the column sums."""
    s = np.asarray(s, dtype=np.int64)
    a = np.einsum("ux,nyx->nyu", T, s)
    a1 = (a + 128) >> 8
    b = np.einsum("vy,nyu->nvu", T, a1)
    return a, a1, b


def quantise(b: np.ndarray, q: np.ndarray) -> np.ndarray:
    """``b [n, 8(v), 8(u)]`` by ``q [n, 8, 8]`` (or ``[8, 8]``): round half away from zero, the clamps of stv.h."""
    d = np.asarray(q, dtype=np.int64) << 18
    raw = np.sign(b) * ((np.abs(b) + (d >> 1)) // d)
    c = np.clip(raw, -1023, 1023)
    c[:, 0, 0] = np.clip(raw[:, 0, 0], -1024, 1023)
    return c


def dct_quant(frame: np.ndarray, qtabs) -> np.ndarray:
    q = np.asarray(qtabs, dtype=np.int64).reshape(2, 8, 8)
    s = samples(frame)
    _, _, b = dct_stages(s)
    tab = (np.arange(len(s)) % 6 >= 4).astype(np.int64)
    c = quantise(b, q[tab]).reshape(-1, 64)
    return np.ascontiguousarray(c[:, list(mjpeg.ZIGZAG)]).astype(np.int16)


def _codes(table) -> dict[int, tuple[int, int]]:
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC = (_codes(mjpeg.DC_LUMA), _codes(mjpeg.DC_CHROMA))
AC = (_codes(mjpeg.AC_LUMA), _codes(mjpeg.AC_CHROMA))


def _value(v: int) -> tuple[int, int]:
    cat = abs(v).bit_length()
    return ((v if v > 0 else v - 1) & ((1 << cat) - 1), cat)


def block_pieces(z: np.ndarray, pred: int, cls: int) -> list[tuple[int, int]]:
    """The (code, length) pieces of one block: 64 coefficients in zigzag order, the DC predictor, the table class."""
    z = [int(v) for v in z]
    bits, cat = _value(z[0] - pred)
    out = [DC[cls][cat], (bits, cat)]
    run = 0
    for v in z[1:]:
        if v == 0:
            run += 1
            continue
        while run >= 16:
            out.append(AC[cls][0xF0])
            run -= 16
        bits, cat = _value(v)
        out += [AC[cls][run << 4 | cat], (bits, cat)]
        run = 0
    if run:
        out.append(AC[cls][0x00])
    return out


def frame_pieces(coefs: np.ndarray) -> list[list[tuple[int, int]]]:
    """Per block of one frame ``[blocks, 64]`` its pieces; the DC predictors run per component through the frame."""
    pred = [0, 0, 0]
    out = []
    for b, z in enumerate(np.asarray(coefs)):
        comp = max(b % 6 - 3, 0)                    # 0: Y, 1: Cb, 2: Cr
        out.append(block_pieces(z, pred[comp], 0 if comp == 0 else 1))
        pred[comp] = int(z[0])
    return out


def block_bits(coefs: np.ndarray) -> np.ndarray:
    return np.array([sum(n for _, n in pieces) for pieces in frame_pieces(coefs)], dtype=np.uint32)


def encode_scan(coefs: np.ndarray) -> bytes:
    text = "".join(format(code, f"0{n}b") for pieces in frame_pieces(coefs) for code, n in pieces if n)
    text += "1" * (-len(text) % 8)
    return int(text, 2).to_bytes(len(text) // 8, "big") if text else b""


def encode_frame(frame: np.ndarray, qtabs) -> bytes:
    """A complete JFIF file of the frame: the twins, ``mjpeg.jpeg_headers`` and ``mjpeg.stuff``."""
    H, W, _ = frame.shape
    return mjpeg.jpeg_headers(H, W, qtabs) + mjpeg.stuff(encode_scan(dct_quant(frame, qtabs))) + mjpeg.EOI


# ---- a RIFF reader for the tests -------------------------------------------------------------------------------------------

def riff_chunks(data: bytes, start: int = 0, end: int | None = None) -> list[dict]:
    """The chunks of ``data[start:end]``: ``{"id", "at" (offset of the chunk header), "size", "data"}``; a ``RIFF`` or ``LIST``
    chunk also has ``"type"`` and ``"children"``.  Raises on a chunk that runs past its parent."""
    end = len(data) if end is None else end
    out, at = [], start
    while at < end:
        assert at + 8 <= end, f"a chunk header at {at} runs past {end}"
        fourcc, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
        assert at + 8 + size <= end, f"chunk {fourcc!r} at {at} of {size} bytes runs past {end}"
        entry = {"id": fourcc, "at": at, "size": size, "data": data[at + 8:at + 8 + size]}
        if fourcc in (b"RIFF", b"LIST"):
            entry["type"] = data[at + 8:at + 12]
            entry["children"] = riff_chunks(data, at + 12, at + 8 + size)
        out.append(entry)
        at += 8 + size + size % 2
    return out


def find(chunks: list[dict], *path: bytes) -> dict:
    """The first chunk along ``path``: list types for lists (``b"hdrl"``), ids for leaves (``b"avih"``)."""
    for entry in chunks:
        if entry.get("type", entry["id"]) == path[0]:
            return entry if len(path) == 1 else find(entry["children"], *path[1:])
    raise KeyError(path)


def read_avi(data: bytes) -> dict:
    """``avih`` and ``strh`` as tuples of integers, ``strf``, the INFO strings, the ``00dc`` chunks and the index entries."""
    (riff,) = riff_chunks(data)
    assert riff["id"] == b"RIFF" and riff["type"] == b"AVI " and riff["size"] == len(data) - 8
    top = riff["children"]
    movi = find(top, b"movi")
    info = {c["id"]: c["data"].rstrip(b"\x00").decode("utf-8") for c in find(top, b"INFO")["children"]}
    idx = find(top, b"idx1")["data"]
    return {
        "avih": struct.unpack("<14I", find(top, b"hdrl", b"avih")["data"]),
        "strh": (find(top, b"hdrl", b"strl", b"strh")["data"][:8], struct.unpack("<IHHIIIIIIII4H", find(top, b"hdrl", b"strl", b"strh")["data"][8:])),
        "strf": struct.unpack("<IiiHH4sIiiII", find(top, b"hdrl", b"strl", b"strf")["data"]),
        "info": info, "movi_at": movi["at"] + 8, "frames": movi["children"],
        "index": [(idx[i:i + 4], *struct.unpack_from("<III", idx, i + 4)) for i in range(0, len(idx), 16)],
    }
