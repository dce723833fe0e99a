// png_read.cpp -- PNG reader for texture images: an inflate (RFC 1950 / 1951) and a PNG
// decoder, both written here (the project links no zlib).  Host only, no HIP call.
//
//   mcpt_image_read_png_memory  a PNG payload (a file's bytes, a glb's bufferView) -> w x h RGBA8, row 0 first
//   mcpt_image_read_png         the same over a file
//   mcpt_image_read_png_error   the reason of this thread's last MCPT_E_IO from either
//
// Accepted: colour type 0 at depth 1/2/4/8/16, 2 at 8/16, 3 at 1/2/4/8 (PLTE, optional tRNS), 4 at 8/16, 6 at
// 8/16; non-interlaced; all five filter types; any number of consecutive IDAT chunks; ancillary chunks skipped;
// w, h in 1..16384.  Conversion: a 16-bit sample becomes its high byte; a grey sample of depth d < 8 becomes
// v * (255 / (2^d - 1)) (255, 85, 17: exact); grey replicates to rgb; alpha is 255 where the file has none (tRNS
// counts for palette images only).  Row 0 of the file is row 0 of the output.
// Everything else is refused with MCPT_E_IO and a message, and nothing is written to the caller's buffer: the
// image is decoded into buffers of this file and copied out only when the whole file has been accepted.
// Every read of the input is bounds-checked; the inflate's output size, h * (1 + rowbytes), is known from IHDR
// before decoding starts, and the stream must yield exactly that (no buffer grows on the stream's say-so).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

#include "mcpt.h"

namespace {

thread_local char g_msg[128] = "";
int fail(const char* why) {
    snprintf(g_msg, sizeof g_msg, "png: %s", why);
    return MCPT_E_IO;
}

// ---------------------------------------------------------------------------------------------
// inflate: stored, fixed and dynamic blocks into a buffer of known size
struct Bits {
    const uint8_t* p;
    size_t n, pos = 0;
    uint32_t acc = 0;
    int cnt = 0;
    bool over = false;  // a read went past the end (the bits read as 0)
    Bits(const uint8_t* d, size_t len) : p(d), n(len) {}
    uint32_t get(int k) {  // k in 0..16, LSB first
        while (cnt < k) {
            if (pos < n) acc |= (uint32_t)p[pos++] << cnt;
            else over = true;
            cnt += 8;
        }
        const uint32_t v = acc & ((1u << k) - 1u);
        acc >>= k;
        cnt -= k;
        return v;
    }
    void align() { acc = 0, cnt = 0; }  // (whole unread bytes never sit in acc: get() fetches one byte at a time)
};

// A canonical Huffman code: how many codes of each length, and the symbols in code order
struct Huff {
    uint16_t count[16];
    uint16_t sym[288];
};
// > 0: incomplete, 0: complete, < 0: over-subscribed (RFC 1951 3.2.2)
int huff_build(Huff& h, const uint8_t* len, int n) {
    memset(h.count, 0, sizeof h.count);
    for (int i = 0; i < n; i++) h.count[len[i]]++;
    int left = 1;
    for (int l = 1; l < 16; l++) {
        left <<= 1;
        left -= h.count[l];
        if (left < 0) return left;
    }
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
    for (int i = 0; i < n; i++)
        if (len[i]) h.sym[offs[len[i]]++] = (uint16_t)i;
    return left;
}
// The next symbol, or -1 when the bits match no code (an incomplete code's unused pattern, or input exhausted)
int huff_decode(Bits& b, const Huff& h) {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; l++) {
        code |= (int)b.get(1);
        if (b.over) return -1;
        const int c = h.count[l];
        if (code - c < first) return h.sym[index + (code - first)];
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

const uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

const char* inflate_codes(Bits& b, const Huff& lit, const Huff& dist, uint8_t* out, size_t cap, size_t& at) {
    for (;;) {
        const int s = huff_decode(b, lit);
        if (s < 0) return b.over ? "deflate stream ends early" : "invalid literal/length code";
        if (s < 256) {
            if (at >= cap) return "deflate stream yields more bytes than the image has";
            out[at++] = (uint8_t)s;
            continue;
        }
        if (s == 256) return nullptr;
        if (s > 285) return "invalid length symbol";
        const size_t len = kLenBase[s - 257] + b.get(kLenExtra[s - 257]);
        const int ds = huff_decode(b, dist);
        if (ds < 0) return b.over ? "deflate stream ends early" : "invalid distance code";
        if (ds > 29) return "invalid distance symbol";
        const size_t d = kDistBase[ds] + b.get(kDistExtra[ds]);
        if (b.over) return "deflate stream ends early";
        if (d > at) return "distance beyond the bytes already produced";
        if (len > cap - at) return "deflate stream yields more bytes than the image has";
        for (size_t k = 0; k < len; k++, at++) out[at] = out[at - d];  // (overlapping copies repeat: byte by byte)
    }
}

const char* inflate_dynamic(Bits& b, Huff& lit, Huff& dist) {
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    const int nlen = (int)b.get(5) + 257, ndist = (int)b.get(5) + 1, ncode = (int)b.get(4) + 4;
    if (b.over) return "deflate stream ends early";
    if (nlen > 286 || ndist > 30) return "too many length or distance codes";
    uint8_t len[286 + 30];
    uint8_t cl[19] = {};
    for (int i = 0; i < ncode; i++) cl[order[i]] = (uint8_t)b.get(3);
    if (b.over) return "deflate stream ends early";
    Huff ch;
    if (huff_build(ch, cl, 19) != 0) return "code-length code over-subscribed or incomplete";
    for (int i = 0; i < nlen + ndist;) {
        const int s = huff_decode(b, ch);
        if (s < 0) return b.over ? "deflate stream ends early" : "invalid code-length code";
        if (s < 16) {
            len[i++] = (uint8_t)s;
            continue;
        }
        uint8_t v = 0;
        int rep;
        if (s == 16) {
            if (i == 0) return "length repeat without a previous length";
            v = len[i - 1];
            rep = 3 + (int)b.get(2);
        } else if (s == 17) {
            rep = 3 + (int)b.get(3);
        } else {
            rep = 11 + (int)b.get(7);
        }
        if (b.over) return "deflate stream ends early";
        if (i + rep > nlen + ndist) return "length repeat beyond the code lengths";
        while (rep--) len[i++] = v;
    }
    if (len[256] == 0) return "no end-of-block code";
    if (huff_build(lit, len, nlen) != 0) return "literal/length code over-subscribed or incomplete";
    const int left = huff_build(dist, len + nlen, ndist);
    if (left < 0) return "distance code over-subscribed";
    if (left > 0) {  // incomplete: RFC 1951 allows one distance code of one bit, and none at all (3.2.7)
        int used = 0;
        for (int l = 1; l < 16; l++) used += dist.count[l];
        if (!(used == 0 || (used == 1 && dist.count[1] == 1))) return "distance code incomplete";
    }
    return nullptr;
}

// The zlib stream z[0 .. n) into exactly `cap` bytes
const char* zlib_inflate(const uint8_t* z, size_t n, uint8_t* out, size_t cap) {
    if (n < 2) return "zlib stream too short";
    if (z[0] != 0x78) return "zlib header is not deflate with a 32K window";
    if (((uint32_t)z[0] * 256u + z[1]) % 31u != 0) return "zlib header check fails";
    if (z[1] & 0x20) return "zlib preset dictionary";
    Bits b(z + 2, n - 2);
    size_t at = 0;
    for (bool last = false; !last;) {
        last = b.get(1) != 0;
        const uint32_t type = b.get(2);
        if (b.over) return "deflate stream ends early";
        if (type == 0) {
            b.align();
            if (b.n - b.pos < 4) return "deflate stream ends early";
            const uint32_t len = b.p[b.pos] | (uint32_t)b.p[b.pos + 1] << 8, nlen = b.p[b.pos + 2] | (uint32_t)b.p[b.pos + 3] << 8;
            b.pos += 4;
            if ((len ^ 0xFFFFu) != nlen) return "stored block: LEN and NLEN disagree";
            if (b.n - b.pos < len) return "deflate stream ends early";
            if (len > cap - at) return "deflate stream yields more bytes than the image has";
            memcpy(out + at, b.p + b.pos, len);
            at += len;
            b.pos += len;
        } else if (type == 1) {
            static thread_local Huff lit, dist;
            uint8_t len[288];
            for (int i = 0; i < 288; i++) len[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
            huff_build(lit, len, 288);
            for (int i = 0; i < 30; i++) len[i] = 5;
            huff_build(dist, len, 30);  // (30 codes of 5 bits: incomplete by 2, as the format defines it)
            if (const char* e = inflate_codes(b, lit, dist, out, cap, at)) return e;
        } else if (type == 2) {
            Huff lit, dist;
            if (const char* e = inflate_dynamic(b, lit, dist)) return e;
            if (const char* e = inflate_codes(b, lit, dist, out, cap, at)) return e;
        } else {
            return "reserved deflate block type";
        }
    }
    if (at != cap) return "deflate stream yields fewer bytes than the image has";
    b.align();
    if (b.n - b.pos < 4) return "no Adler-32";
    const uint32_t want = (uint32_t)b.p[b.pos] << 24 | (uint32_t)b.p[b.pos + 1] << 16 | (uint32_t)b.p[b.pos + 2] << 8 | b.p[b.pos + 3];
    uint32_t s1 = 1, s2 = 0;
    for (size_t i = 0; i < cap;) {
        const size_t end = cap - i < 5552 ? cap : i + 5552;  // (5552 bytes keep both sums below 2^32)
        for (; i < end; i++) s1 += out[i], s2 += s1;
        s1 %= 65521u, s2 %= 65521u;
    }
    if (((s2 << 16) | s1) != want) return "bad Adler-32";
    return nullptr;
}

// ---------------------------------------------------------------------------------------------
// PNG
uint32_t crc32(const uint8_t* p, size_t n) {
    static uint32_t table[256];
    static bool ready = [] {
        for (uint32_t k = 0; k < 256; k++) {
            uint32_t c = k;
            for (int j = 0; j < 8; j++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[k] = c;
        }
        return true;
    }();
    (void)ready;
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) c = table[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}
uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

struct Header {
    int32_t w = 0, h = 0;
    int depth = 0, type = 0, channels = 0;
};

// Signature and IHDR; *at is left behind the IHDR chunk
int read_header(const uint8_t* d, size_t n, Header& hd, size_t& at) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (n < 8 || memcmp(d, sig, 8) != 0) return fail("bad signature");
    if (n < 8 + 25) return fail("file ends inside IHDR");
    if (be32(d + 8) != 13 || memcmp(d + 12, "IHDR", 4) != 0) return fail("the first chunk is not IHDR");
    if (crc32(d + 12, 17) != be32(d + 29)) return fail("bad chunk CRC (IHDR)");
    const uint8_t* p = d + 16;
    const uint32_t w = be32(p), h = be32(p + 4);
    if (w < 1 || w > 16384 || h < 1 || h > 16384) return fail("width and height must be 1..16384");
    hd.w = (int32_t)w, hd.h = (int32_t)h, hd.depth = p[8], hd.type = p[9];
    const int dp = hd.depth;
    bool ok = false;
    switch (hd.type) {
        case 0: hd.channels = 1, ok = dp == 1 || dp == 2 || dp == 4 || dp == 8 || dp == 16; break;
        case 2: hd.channels = 3, ok = dp == 8 || dp == 16; break;
        case 3: hd.channels = 1, ok = dp == 1 || dp == 2 || dp == 4 || dp == 8; break;
        case 4: hd.channels = 2, ok = dp == 8 || dp == 16; break;
        case 6: hd.channels = 4, ok = dp == 8 || dp == 16; break;
        default: break;
    }
    if (!ok) return fail("colour type and bit depth do not go together");
    if (p[10] != 0) return fail("unknown compression method");
    if (p[11] != 0) return fail("unknown filter method");
    if (p[12] == 1) return fail("Adam7 interlace is not supported");
    if (p[12] != 0) return fail("unknown interlace method");
    at = 8 + 25;
    return MCPT_OK;
}

int decode(const uint8_t* d, size_t n, const Header& hd, size_t at, std::vector<uint8_t>& rgba) {
    uint8_t pal[256][4];
    int npal = 0;
    bool seen_plte = false, seen_trns = false, seen_idat = false, idat_over = false, seen_end = false;
    std::vector<uint8_t> z;
    while (!seen_end) {
        if (n - at < 12) return fail("file ends before IEND");
        const uint32_t len = be32(d + at);
        if (len > n - at - 12) return fail("chunk longer than the file");
        const uint8_t* type = d + at + 4;
        const uint8_t* data = d + at + 8;
        if (crc32(type, 4 + (size_t)len) != be32(data + len)) return fail("bad chunk CRC");
        at += 12 + (size_t)len;
        const bool idat = memcmp(type, "IDAT", 4) == 0;
        if (seen_idat && !idat) idat_over = true;
        if (idat) {
            if (idat_over) return fail("IDAT chunks are not consecutive");
            if (hd.type == 3 && !seen_plte) return fail("palette image without PLTE before IDAT");
            seen_idat = true;
            z.insert(z.end(), data, data + len);  // (bounded by the file's size)
        } else if (memcmp(type, "IHDR", 4) == 0) {
            return fail("a second IHDR");
        } else if (memcmp(type, "PLTE", 4) == 0) {
            if (seen_plte || seen_idat || seen_trns) return fail("PLTE out of order");
            if (hd.type == 0 || hd.type == 4) return fail("PLTE in a greyscale image");
            if (len == 0 || len % 3 != 0 || len > 768) return fail("bad PLTE length");
            seen_plte = true;
            npal = (int)(len / 3);
            for (int k = 0; k < npal; k++) pal[k][0] = data[3 * k], pal[k][1] = data[3 * k + 1], pal[k][2] = data[3 * k + 2], pal[k][3] = 255;
        } else if (memcmp(type, "tRNS", 4) == 0) {
            if (seen_trns || seen_idat) return fail("tRNS out of order");
            seen_trns = true;
            if (hd.type == 3) {  // (tRNS counts for palette images only)
                if (!seen_plte) return fail("tRNS before PLTE");
                if ((int)len > npal) return fail("tRNS longer than PLTE");
                for (uint32_t k = 0; k < len; k++) pal[k][3] = data[k];
            }
        } else if (memcmp(type, "IEND", 4) == 0) {
            if (!seen_idat) return fail("IEND before IDAT");
            if (len != 0) return fail("bad IEND length");
            seen_end = true;
        } else if (!(type[0] & 0x20)) {
            return fail("unknown critical chunk");
        }  // (an ancillary chunk: skipped, its CRC checked)
    }
    const size_t bits = (size_t)hd.channels * hd.depth;
    const size_t rowbytes = ((size_t)hd.w * bits + 7) / 8, bpp = bits >= 8 ? bits / 8 : 1;
    std::vector<uint8_t> raw((size_t)hd.h * (1 + rowbytes));
    if (const char* e = zlib_inflate(z.data(), z.size(), raw.data(), raw.size())) return fail(e);
    // unfilter in place (PNG 9.2); the row above the first is zeros
    for (int32_t y = 0; y < hd.h; y++) {
        uint8_t* r = raw.data() + (size_t)y * (1 + rowbytes) + 1;
        const uint8_t* up = y ? r - (1 + rowbytes) : nullptr;
        const uint8_t f = r[-1];
        if (f > 4) return fail("unknown filter type");
        for (size_t i = 0; i < rowbytes; i++) {
            const int a = i >= bpp ? r[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= bpp) ? up[i - bpp] : 0;
            const int add = f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? (a + b) / 2 : paeth(a, b, c);
            r[i] = (uint8_t)(r[i] + add);
        }
    }
    rgba.resize((size_t)hd.w * hd.h * 4);
    const int step = hd.depth == 16 ? 2 : 1;  // a 16-bit sample becomes its high byte
    for (int32_t y = 0; y < hd.h; y++) {
        const uint8_t* r = raw.data() + (size_t)y * (1 + rowbytes) + 1;
        uint8_t* o = rgba.data() + (size_t)y * hd.w * 4;
        for (int32_t x = 0; x < hd.w; x++, o += 4) {
            if (hd.depth < 8) {  // grey or palette index, packed from the high bits down
                const size_t bit = (size_t)x * hd.depth;
                const int v = (r[bit >> 3] >> (8 - hd.depth - (int)(bit & 7))) & ((1 << hd.depth) - 1);
                if (hd.type == 3) {
                    if (v >= npal) return fail("palette index beyond PLTE");
                    memcpy(o, pal[v], 4);
                } else {
                    o[0] = o[1] = o[2] = (uint8_t)(v * (255 / ((1 << hd.depth) - 1)));
                    o[3] = 255;
                }
                continue;
            }
            const uint8_t* s = r + (size_t)x * hd.channels * step;
            switch (hd.type) {
                case 0: o[0] = o[1] = o[2] = s[0], o[3] = 255; break;
                case 2: o[0] = s[0], o[1] = s[step], o[2] = s[2 * step], o[3] = 255; break;
                case 3:
                    if (s[0] >= npal) return fail("palette index beyond PLTE");
                    memcpy(o, pal[s[0]], 4);
                    break;
                case 4: o[0] = o[1] = o[2] = s[0], o[3] = s[step]; break;
                default: o[0] = s[0], o[1] = s[step], o[2] = s[2 * step], o[3] = s[3 * step]; break;
            }
        }
    }
    return MCPT_OK;
}

}  // namespace

extern "C" {

int mcpt_image_read_png_memory(const uint8_t* data, size_t n, int32_t* w, int32_t* h, uint8_t* rgba8, size_t cap) {
    if (!data || !w || !h) return MCPT_E_INVALID;
    Header hd;
    size_t at = 0;
    if (int rc = read_header(data, n, hd, at)) return rc;
    if (!rgba8) {  // the size alone, from a valid IHDR (the rest of the file is not looked at)
        *w = hd.w, *h = hd.h;
        return MCPT_OK;
    }
    if (cap < (size_t)hd.w * (size_t)hd.h * 4) return MCPT_E_INVALID;
    try {  // (the decoder's buffers follow IHDR: up to 3 GiB for a 16384 x 16384 16-bit RGBA image)
        std::vector<uint8_t> rgba;
        if (int rc = decode(data, n, hd, at, rgba)) return rc;
        *w = hd.w, *h = hd.h;
        memcpy(rgba8, rgba.data(), rgba.size());
    } catch (const std::bad_alloc&) {
        snprintf(g_msg, sizeof g_msg, "png: out of memory");
        return MCPT_E_NOMEM;
    }
    return MCPT_OK;
}

int mcpt_image_read_png(const char* path, int32_t* w, int32_t* h, uint8_t* rgba8, size_t cap) {
    if (!path || !w || !h) return MCPT_E_INVALID;
    FILE* f = fopen(path, "rb");
    if (!f) return fail("cannot read the file");
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    size_t got;
    bool bad = false;
    try {
        while ((got = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + got);
    } catch (const std::bad_alloc&) {
        fclose(f);
        snprintf(g_msg, sizeof g_msg, "png: out of memory");
        return MCPT_E_NOMEM;
    }
    bad = ferror(f) != 0;
    fclose(f);
    if (bad) return fail("cannot read the file");
    if (d.empty()) return fail("bad signature");
    return mcpt_image_read_png_memory(d.data(), d.size(), w, h, rgba8, cap);
}

const char* mcpt_image_read_png_error(void) { return g_msg; }

}  // extern "C"
