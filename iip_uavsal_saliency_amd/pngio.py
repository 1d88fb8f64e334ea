"""8-bit greyscale PNG on the standard library's zlib: what `cv2.imwrite(path, grey)` / `cv2.imread(path, 0)` exchange
for the reference's `priors/<video>.png` (utils_data.py:520, 571), so that a dataset's `priors/` folder written here can be
read by the reference and the other way round.

`write_gray` emits one IDAT, non-interlaced, every row with filter 0.  `read_gray` undoes the filters 0-4 (a file cv2
wrote uses them) of a non-interlaced 8-bit greyscale file; colour, palette, alpha, 16-bit and interlaced files raise
`ValueError` -- nothing is converted silently.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

_SIG = b"\x89PNG\r\n\x1a\n"


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def encode_gray(img: np.ndarray) -> bytes:
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("encode_gray: expected a non-empty 2-d uint8 image, got %s %r" % (img.dtype, img.shape))
    h, w = img.shape
    rows = np.zeros((h, w + 1), dtype=np.uint8)            # a filter byte (0) in front of every row
    rows[:, 1:] = img
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)
    return _SIG + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b"")


def write_gray(path: str, img: np.ndarray) -> None:
    data = encode_gray(img)
    with open(path, "wb") as f:
        f.write(data)


def decode_gray(data: bytes) -> np.ndarray:
    if data[:8] != _SIG:
        raise ValueError("not a PNG file")
    pos, ihdr, idat, ended = 8, None, [], False
    while pos + 8 <= len(data) and not ended:
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if len(body) != n or pos + 12 + n > len(data):
            raise ValueError("truncated PNG chunk %r" % kind)
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(kind + body) & 0xffffffff):
            raise ValueError("PNG chunk %r fails its CRC" % kind)
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
        pos += 12 + n
    if ihdr is None or not idat or not ended:
        raise ValueError("PNG without IHDR / IDAT / IEND")
    w, h, depth, colour, comp, filt, interlace = ihdr
    if colour != 0 or depth != 8:
        raise ValueError("only 8-bit greyscale PNG is read (colour type %d, bit depth %d)" % (colour, depth))
    if interlace != 0 or comp != 0 or filt != 0:
        raise ValueError("interlaced PNG (or an unknown compression / filter method) is not read")
    raw = zlib.decompress(b"".join(idat))
    if w < 1 or h < 1 or len(raw) != h * (w + 1):
        raise ValueError("PNG data are %d bytes, %d rows of 1 + %d expected" % (len(raw), h, w))
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, w + 1)
    out = np.zeros((h, w), dtype=np.uint8)
    prev = np.zeros(w, dtype=np.int64)
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        if ft == 0:
            cur = line
        elif ft == 2:                                      # Up
            cur = (line + prev) & 255
        elif ft == 1:                                      # Sub: a running sum modulo 256
            cur = np.cumsum(line) & 255
        elif ft in (3, 4):                                 # Average / Paeth: each byte needs its left neighbour
            cur = np.zeros(w, dtype=np.int64)
            left = up_left = 0
            for x in range(w):
                up = int(prev[x])
                if ft == 3:
                    pred = (left + up) >> 1
                else:
                    p = left + up - up_left
                    pa, pb, pc = abs(p - left), abs(p - up), abs(p - up_left)
                    pred = left if (pa <= pb and pa <= pc) else (up if pb <= pc else up_left)
                left = (int(line[x]) + pred) & 255
                cur[x] = left
                up_left = up
        else:
            raise ValueError("PNG row %d has filter type %d" % (y, ft))
        out[y] = cur
        prev = cur
    return out


def read_gray(path: str) -> np.ndarray:
    with open(path, "rb") as f:
        return decode_gray(f.read())
