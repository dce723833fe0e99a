"""PNG files from arrays, written with Python's zlib and struct (no imaging library): the inputs of
tests/test_png_read_host.py.

write(px, ...) takes samples as the file stores them, an (h, w, channels) array of uint8 (depth <= 8; values
below 2 ** depth) or uint16 (depth 16), with a choice of colour type and bit depth, filter per row, zlib level
(0: stored blocks) and strategy (zlib.Z_FIXED: fixed Huffman blocks), IDAT split size, and the interlace flag.
expected(px, ...) is the RGBA8 image mcpt_image_read_png* must return for that file under the conversion rules
of include/mcpt.h."""
import struct
import zlib

import numpy as np

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
ACCEPTED = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
SIG = b"\x89PNG\r\n\x1a\n"


def chunk(kind, data, crc=None):
    c = zlib.crc32(kind + data) & 0xFFFFFFFF if crc is None else crc
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", c)


def pack_rows(px, depth):
    """(h, rowbytes) uint8: the samples of each row packed as PNG packs them (big-endian 16-bit, high bits first)."""
    px = np.asarray(px)
    h, w, ch = px.shape
    if depth == 16:
        return np.ascontiguousarray(px.astype(">u2")).view(np.uint8).reshape(h, w * ch * 2)
    if depth == 8:
        return px.astype(np.uint8).reshape(h, w * ch)
    bits = np.zeros((h, ((w * depth + 7) // 8) * 8), np.uint8)
    v = px.reshape(h, w).astype(np.uint8)
    for b in range(depth):
        bits[:, b:w * depth:depth] = (v >> (depth - 1 - b)) & 1
    return np.packbits(bits, axis=1)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(rows, bpp, filters):
    """The filtered scanlines, each with its filter-type byte in front (PNG 9.2)."""
    h, n = rows.shape
    out = bytearray()
    prev = np.zeros(n, np.int32)
    for y in range(h):
        f = filters[y % len(filters)]
        cur = rows[y].astype(np.int32)
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        if f == 0:
            pred = np.zeros(n, np.int32)
        elif f == 1:
            pred = a
        elif f == 2:
            pred = prev
        elif f == 3:
            pred = (a + prev) // 2
        else:
            pred = _paeth(a, prev, c)
        out.append(f)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return c.compress(raw) + c.flush()


def write(px, ctype=6, depth=8, filters=(0,), level=6, strategy=zlib.Z_DEFAULT_STRATEGY, idat=None, interlace=0, palette=None,
          trns=None, extra=(), zdata=None):
    """PNG bytes.  px: (h, w, CHANNELS[ctype]) samples (indices for ctype 3).  filters: the filter type of row y
    is filters[y % len(filters)].  idat: split the compressed stream into IDAT chunks of that many bytes (None:
    one chunk).  palette: (n, 3) uint8 and trns: (m,) uint8 for ctype 3 (trns is written for any type when
    given).  extra: chunks (kind, data) put between IHDR and PLTE.  zdata: the zlib stream to store in place of
    the compressed scanlines."""
    px = np.asarray(px)
    h, w, ch = px.shape
    assert ch == CHANNELS[ctype]
    rows = pack_rows(px, depth)
    bpp = max(1, ch * depth // 8)
    z = deflate(filter_rows(rows, bpp, filters), level, strategy) if zdata is None else zdata
    out = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))
    for kind, data in extra:
        out += chunk(kind, data)
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    if trns is not None:
        out += chunk(b"tRNS", np.asarray(trns, np.uint8).tobytes())
    step = len(z) if not idat else idat
    for k in range(0, max(len(z), 1), max(step, 1)):
        out += chunk(b"IDAT", z[k:k + step])
    return out + chunk(b"IEND", b"")


def expected(px, ctype=6, depth=8, palette=None, trns=None):
    """(h, w, 4) uint8: the conversion rules.  A 16-bit sample becomes its high byte, a grey sample of depth
    d < 8 becomes v * (255 // (2 ** d - 1)), grey replicates to rgb, alpha is 255 where the file has none, tRNS
    counts for palette images only."""
    px = np.asarray(px)
    h, w, _ = px.shape
    v = (px >> 8).astype(np.uint8) if depth == 16 else px.astype(np.uint8)
    out = np.full((h, w, 4), 255, np.uint8)
    if ctype == 3:
        pal = np.full((256, 4), 255, np.uint8)
        p = np.asarray(palette, np.uint8)
        pal[:len(p), :3] = p
        if trns is not None:
            pal[:len(trns), 3] = np.asarray(trns, np.uint8)
        return pal[v[..., 0]]
    if ctype in (0, 4):
        g = v[..., 0] * (255 // ((1 << depth) - 1)) if depth < 8 else v[..., 0]
        out[..., 0] = out[..., 1] = out[..., 2] = g
        if ctype == 4:
            out[..., 3] = v[..., 1]
        return out
    out[..., :v.shape[2]] = v
    return out


def random_samples(rng, h, w, ctype, depth, npal=None):
    """Random samples for a type and depth (palette indices below npal)."""
    ch = CHANNELS[ctype]
    if depth == 16:
        return rng.integers(0, 65536, (h, w, ch)).astype(np.uint16)
    hi = (1 << depth) if ctype != 3 else min(1 << depth, npal)
    return rng.integers(0, hi, (h, w, ch)).astype(np.uint8)
