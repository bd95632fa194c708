// jpeg_entropy.hpp -- the host half of the JPEG decode: marker parser + Huffman entropy decoder, plain C++17.
//
// No HIP, no globals, no allocation (the parsed headers live in the caller's JeStream, the decoder's look-up tables -- 36 KB, built only for the tables the scan uses -- on je_decode's stack), re-entrant.  Included by
// frame_jpeg.hip for the C-ABI and by tests/jpeg_entropy_main.cpp for the stand-alone sanitizer program.
//
// Supported: 8-bit baseline (SOF0) and extended-sequential Huffman (SOF1) streams with ONE interleaved scan; 1 component
// (grey) or 3 components YCbCr (JFIF marker, or Adobe marker with transform 1, or neither marker and component ids that
// are not 'R','G','B' -- libjpeg's rule) with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; 8- and 16-bit DQT; DRI with
// RST0..7; 0xFF00 stuffing, fill bytes, APPn / COM.  Everything else that is a well-formed JPEG header (progressive,
// arithmetic, lossless, 12-bit, 2 or 4 components, RGB-coded, other sampling factors, a scan over some of the components,
// sides above 10752) is JE_NOTIMPL, decided before any coefficient is produced; malformed or truncated data is JE_BADARG.
// So is a coefficient whose product with its quantiser does not fit 16 bits (|c q| > 32767): no encoder of 8-bit samples
// writes one (the products stay below about 2^11 q / 2), libjpeg-turbo's own vector IDCT holds the products in int16, and
// the device stage's 32-bit IDCT is specified for such inputs only.
// Nothing is read outside [data, data + len) or written outside the packed frame.
//
// Packed frame (also documented in include/meshraster_hip.h):
//   bytes   0 ..  63  int32 header[16]: magic, width, height, components, luma_h, luma_v, tq[3] (quantisation table of each
//                     component), restart interval, packed bytes (low 32 bits), zeros
//   bytes  64 .. 575  four quantisation tables, u16[64] each, natural (row-major) order; tables the stream does not define
//                     are zeros
//   bytes 576 ..      the coefficients, int16[64] per block in natural order: component after component, each component's
//                     blocks row-major over its plane padded to whole MCUs
#ifndef MR_JPEG_ENTROPY_HPP
#define MR_JPEG_ENTROPY_HPP

#include <stdint.h>
#include <string.h>

namespace mrjpeg {

constexpr int JE_OK = 0, JE_BADARG = -1, JE_NOTIMPL = -2;
constexpr int JE_MAGIC = 0x314A524D;  // "MRJ1"
constexpr int JE_HEADER_BYTES = 576;  // header + four quantisation tables; the coefficients start here
constexpr int JE_MAX_DIM = 10752;     // mr_frames_color_augment's limit

static const uint8_t JE_NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JeGeometry {
    int width, height, ncomp, hl, vl;  // hl, vl: luma sampling (1 for grey)
    int mcus_x, mcus_y;
    int bw[3], bh[3];                  // blocks across / down each component's padded plane
    int64_t block_base[3];             // first block of each component
    int64_t blocks;                    // blocks of a frame
};

// geometry of a supported frame; false for anything else
inline bool je_geometry(int width, int height, int ncomp, int hl, int vl, JeGeometry& g) {
    if (width < 1 || height < 1 || width > JE_MAX_DIM || height > JE_MAX_DIM) return false;
    if (ncomp == 1) {
        if (hl != 1 || vl != 1) return false;
    } else if (ncomp == 3) {
        if (!((hl == 1 && vl == 1) || (hl == 2 && vl == 1) || (hl == 2 && vl == 2))) return false;
    } else {
        return false;
    }
    g.width = width; g.height = height; g.ncomp = ncomp; g.hl = hl; g.vl = vl;
    g.mcus_x = (width + 8 * hl - 1) / (8 * hl);
    g.mcus_y = (height + 8 * vl - 1) / (8 * vl);
    g.blocks = 0;
    for (int c = 0; c < 3; c++) {
        const int h = c == 0 ? hl : 1, v = c == 0 ? vl : 1;
        g.bw[c] = c < ncomp ? g.mcus_x * h : 0;
        g.bh[c] = c < ncomp ? g.mcus_y * v : 0;
        g.block_base[c] = g.blocks;
        g.blocks += (int64_t)g.bw[c] * g.bh[c];
    }
    return true;
}

inline int64_t je_packed_bytes(int width, int height, int ncomp, int hl, int vl) {
    JeGeometry g;
    if (!je_geometry(width, height, ncomp, hl, vl, g)) return -1;
    return JE_HEADER_BYTES + 128 * g.blocks;
}

struct JeHuff {
    bool defined;
    uint16_t lut[1024];   // 10 leading bits -> (length << 8 | symbol); 0: the code is longer than 10 bits
    int16_t fast[1024];   // AC: 10 leading bits -> (value << 8 | run << 4 | code + value bits) where a code and its value fit
                          // them and the value fits 8 bits; 0: take the long way
    int32_t maxcode[18];  // largest code of each length (-1: none)
    int32_t valoff[17];   // index of a length's first symbol minus its first code
    uint8_t vals[256];
};

struct JeStream {
    JeGeometry g;
    int restart;          // MCUs between restart markers (0: none)
    int tq[3], td[3], ta[3];
    bool qdefined[4];
    uint16_t q[4][64];    // natural order
    int64_t dht[2][4];    // offset of each DC / AC table's 16 counts in the data (-1: not defined); validated by je_parse
    int64_t scan;         // offset of the first entropy-coded byte
};

inline int je_build_huff(JeHuff& h, const uint8_t* counts, const uint8_t* symbols, int total) {
    memset(h.lut, 0, sizeof(h.lut));
    memcpy(h.vals, symbols, (size_t)total);
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; l++) {
        const int n = counts[l - 1];
        h.valoff[l] = k - code;
        if (code + n > (1 << l)) return JE_BADARG;  // more codes of this length than the code space has left
        for (int i = 0; i < n; i++, k++, code++) {
            if (l <= 10) {
                const int first = code << (10 - l);
                for (int f = 0; f < (1 << (10 - l)); f++) h.lut[first + f] = (uint16_t)((l << 8) | symbols[k]);
            }
        }
        h.maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    for (int i = 0; i < 1024; i++) {
        h.fast[i] = 0;
        const int l = h.lut[i] >> 8, run = (h.lut[i] >> 4) & 15, size = h.lut[i] & 15;
        if (l == 0 || size == 0 || l + size > 10) continue;
        const int r = (i >> (10 - l - size)) & ((1 << size) - 1);
        const int v = r < (1 << (size - 1)) ? r - (1 << size) + 1 : r;
        if (v >= -128 && v <= 127) h.fast[i] = (int16_t)(v * 256 + run * 16 + l + size);
    }
    h.defined = true;
    return JE_OK;
}

// Parse the markers up to and including SOS.  JE_NOTIMPL as soon as the headers show an unsupported stream.
inline int je_parse(const uint8_t* data, int64_t len, JeStream& s) {
    if (!data || len < 4 || data[0] != 0xFF || data[1] != 0xD8) return JE_BADARG;
    memset(&s.g, 0, sizeof(s.g));
    s.restart = 0;
    for (int t = 0; t < 4; t++) {
        s.qdefined[t] = false;
        s.dht[0][t] = s.dht[1][t] = -1;
    }
    memset(s.q, 0, sizeof(s.q));
    bool sof = false, jfif = false, adobe = false;
    int adobe_transform = 0, precision = 0, width = 0, height = 0, ncomp = 0;
    int cid[4] = {0, 0, 0, 0}, ch[4] = {0, 0, 0, 0}, cv[4] = {0, 0, 0, 0}, ctq[4] = {0, 0, 0, 0};
    int64_t p = 2;
    for (;;) {
        if (p >= len || data[p] != 0xFF) return JE_BADARG;
        while (p < len && data[p] == 0xFF) p++;  // fill bytes
        if (p >= len) return JE_BADARG;
        const int m = data[p++];
        if (m == 0x01) continue;                             // TEM: stands alone
        if (m == 0x00 || m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7)) return JE_BADARG;
        if (p + 2 > len) return JE_BADARG;
        const int64_t L = (data[p] << 8) | data[p + 1];
        if (L < 2 || p + L > len) return JE_BADARG;
        const uint8_t* d = data + p + 2;
        const int64_t n = L - 2;
        p += L;
        if (m == 0xC0 || m == 0xC1) {
            if (sof || n < 6) return JE_BADARG;
            precision = d[0];
            height = (d[1] << 8) | d[2];
            width = (d[3] << 8) | d[4];
            ncomp = d[5];
            if (ncomp < 1 || ncomp > 4 || n != 6 + 3 * ncomp || width == 0) return JE_BADARG;
            if (precision != 8 && precision != 12) return JE_BADARG;
            for (int c = 0; c < ncomp; c++) {
                cid[c] = d[6 + 3 * c];
                ch[c] = d[7 + 3 * c] >> 4;
                cv[c] = d[7 + 3 * c] & 15;
                ctq[c] = d[8 + 3 * c];
                if (ch[c] < 1 || ch[c] > 4 || cv[c] < 1 || cv[c] > 4 || ctq[c] > 3) return JE_BADARG;
            }
            if (precision != 8 || height == 0) return JE_NOTIMPL;  // 12-bit samples; a height left to a DNL marker
            if (ncomp != 1 && ncomp != 3) return JE_NOTIMPL;
            sof = true;
        } else if ((m >= 0xC2 && m <= 0xCF) && m != 0xC4) {
            return JE_NOTIMPL;  // progressive, lossless, differential, arithmetic (SOFn, JPG, DAC)
        } else if (m == 0xC4) {
            int64_t o = 0;
            while (o < n) {
                if (o + 17 > n) return JE_BADARG;
                const int tc = d[o] >> 4, th = d[o] & 15;
                if (tc > 1 || th > 3) return JE_BADARG;
                int total = 0;
                for (int i = 0; i < 16; i++) total += d[o + 1 + i];
                if (total > 256 || o + 17 + total > n) return JE_BADARG;
                int32_t code = 0;
                for (int l = 1; l <= 16; l++) {  // more codes of a length than the code space has left?
                    code += d[o + l];
                    if (code > (1 << l)) return JE_BADARG;
                    code <<= 1;
                }
                s.dht[tc][th] = (d + o + 1) - data;
                o += 17 + total;
            }
        } else if (m == 0xDB) {
            int64_t o = 0;
            while (o < n) {
                const int pq = d[o] >> 4, tq = d[o] & 15;
                if (pq > 1 || tq > 3 || o + 1 + 64 * (pq + 1) > n) return JE_BADARG;
                for (int i = 0; i < 64; i++)
                    s.q[tq][JE_NATURAL[i]] = pq ? (uint16_t)((d[o + 1 + 2 * i] << 8) | d[o + 2 + 2 * i]) : d[o + 1 + i];
                s.qdefined[tq] = true;
                o += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xDD) {
            if (n != 2) return JE_BADARG;
            s.restart = (d[0] << 8) | d[1];
        } else if (m == 0xE0) {
            if (n >= 14 && memcmp(d, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (n >= 12 && memcmp(d, "Adobe", 5) == 0) {
                adobe = true;
                adobe_transform = d[11];
            }
        } else if (m == 0xDA) {
            if (!sof || n < 1) return JE_BADARG;
            const int ns = d[0];
            if (ns < 1 || ns > 4 || n != 4 + 2 * ns) return JE_BADARG;
            for (int c = 0; c < ns; c++) {
                bool known = false;
                for (int k = 0; k < ncomp; k++) known = known || cid[k] == d[1 + 2 * c];
                if (!known || (d[2 + 2 * c] >> 4) > 3 || (d[2 + 2 * c] & 15) > 3) return JE_BADARG;
            }
            if (ns != ncomp) return JE_NOTIMPL;  // several scans
            for (int c = 0; c < ns; c++) {
                if (d[1 + 2 * c] != cid[c]) return JE_NOTIMPL;  // interleaved in another order than the frame's
                s.td[c] = d[2 + 2 * c] >> 4;
                s.ta[c] = d[2 + 2 * c] & 15;
            }
            if (d[1 + 2 * ns] != 0 || d[2 + 2 * ns] != 63 || d[3 + 2 * ns] != 0) return JE_BADARG;
            break;
        } else if ((m >= 0xE1 && m <= 0xEF) || m == 0xFE || m == 0xDC) {
            // APPn, COM, DNL: skipped
        } else {
            return JE_BADARG;
        }
    }
    // the colour space as libjpeg's default_decompress_parms chooses it
    if (ncomp == 3) {
        if (jfif) {
        } else if (adobe) {
            if (adobe_transform != 1) return JE_NOTIMPL;  // 0: RGB
        } else if (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B') {
            return JE_NOTIMPL;
        }
        if (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1) return JE_NOTIMPL;
    } else {
        ch[0] = cv[0] = 1;  // a one-component scan is not interleaved: one block per MCU whatever the factors say
    }
    if (width > JE_MAX_DIM || height > JE_MAX_DIM) return JE_NOTIMPL;
    if (!je_geometry(width, height, ncomp, ch[0], cv[0], s.g)) return JE_NOTIMPL;
    for (int c = 0; c < 3; c++) {
        if (c >= ncomp) {
            s.tq[c] = s.td[c] = s.ta[c] = 0;
            continue;
        }
        s.tq[c] = ctq[c];
        if (!s.qdefined[s.tq[c]] || s.dht[0][s.td[c]] < 0 || s.dht[1][s.ta[c]] < 0) return JE_BADARG;
    }
    s.scan = p;
    return JE_OK;
}

// MSB-first bit reader over the entropy-coded segment.  A marker (or the end of the data) stops it: from there on it
// supplies zero bits and counts them in `pad`; a block that consumed one of them makes the stream JE_BADARG.
struct JeBits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc;
    int bits, pad;
    bool stopped;
};

inline void je_fill(JeBits& b) {
    if (!b.stopped && b.bits <= 32 && b.end - b.p >= 4) {  // four bytes at once where none of them is 0xFF
        const uint32_t w = ((uint32_t)b.p[0] << 24) | ((uint32_t)b.p[1] << 16) | ((uint32_t)b.p[2] << 8) | b.p[3];
        const uint32_t inv = ~w;
        if (((inv - 0x01010101u) & ~inv & 0x80808080u) == 0) {
            b.acc = (b.acc << 32) | w;
            b.bits += 32;
            b.p += 4;
        }
    }
    while (b.bits <= 56) {
        unsigned byte = 0;
        if (!b.stopped && b.p < b.end) {
            byte = *b.p;
            if (byte == 0xFF) {
                if (b.p + 1 < b.end && b.p[1] == 0x00) {
                    b.p += 2;
                } else {
                    b.stopped = true;
                    byte = 0;
                    b.pad += 8;
                }
            } else {
                b.p++;
            }
        } else {
            b.stopped = true;
            b.pad += 8;
        }
        b.acc = (b.acc << 8) | byte;
        b.bits += 8;
    }
}

inline unsigned je_peek(const JeBits& b, int n) { return (unsigned)(b.acc >> (b.bits - n)) & ((1u << n) - 1u); }

// one Huffman symbol, or -1 for a bit pattern that is no code; at least 16 bits are in the accumulator
inline int je_symbol(JeBits& b, const JeHuff& h) {
    const unsigned e = h.lut[je_peek(b, 10)];
    if (e) {
        b.bits -= (int)(e >> 8);
        return (int)(e & 255);
    }
    const int32_t v = (int32_t)je_peek(b, 16);
    for (int l = 11; l <= 16; l++) {
        const int32_t code = v >> (16 - l);
        if (code <= h.maxcode[l]) {
            const int32_t i = code + h.valoff[l];
            if (i < 0 || i > 255) return -1;
            b.bits -= l;
            return h.vals[i];
        }
    }
    return -1;
}

inline int je_receive_extend(JeBits& b, int s) {
    const int r = (int)je_peek(b, s);
    b.bits -= s;
    return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
}

// Entropy-decode a parsed stream into `packed` (je_packed_bytes(...) bytes).
inline int je_decode(const uint8_t* data, int64_t len, const JeStream& s, uint8_t* packed, int64_t packed_bytes) {
    const JeGeometry& g = s.g;
    const int64_t need = JE_HEADER_BYTES + 128 * g.blocks;
    if (!packed || packed_bytes != need) return JE_BADARG;
    memset(packed, 0, (size_t)need);
    int32_t header[16] = {JE_MAGIC, g.width, g.height, g.ncomp, g.hl, g.vl, s.tq[0], s.tq[1], s.tq[2], s.restart,
                          (int32_t)(uint32_t)need, 0, 0, 0, 0, 0};
    memcpy(packed, header, 64);
    memcpy(packed + 64, s.q, 512);
    int16_t* coef = reinterpret_cast<int16_t*>(packed + JE_HEADER_BYTES);  // (the caller's buffer: 2-byte aligned, see below)
    JeHuff dcs[4], acs[4];  // only the tables the scan names are built
    for (int t = 0; t < 4; t++) dcs[t].defined = acs[t].defined = false;
    for (int c = 0; c < g.ncomp; c++) {
        for (int k = 0; k < 2; k++) {
            JeHuff& h = k ? acs[s.ta[c]] : dcs[s.td[c]];
            if (h.defined) continue;
            const uint8_t* counts = data + s.dht[k][k ? s.ta[c] : s.td[c]];
            int total = 0;
            for (int i = 0; i < 16; i++) total += counts[i];
            if (je_build_huff(h, counts, counts + 16, total) != JE_OK) return JE_BADARG;
        }
    }
    int lim[3][64];  // largest |coefficient| whose product with its quantiser fits 16 bits, natural order
    for (int c = 0; c < g.ncomp; c++)
        for (int i = 0; i < 64; i++) lim[c][i] = s.q[s.tq[c]][i] ? 32767 / s.q[s.tq[c]][i] : 32767;
    JeBits b = {data + s.scan, data + len, 0, 0, 0, false};
    int dcpred[3] = {0, 0, 0};
    int64_t todo = s.restart;
    int next_rst = 0;
    for (int my = 0; my < g.mcus_y; my++) {
        for (int mx = 0; mx < g.mcus_x; mx++) {
            if (s.restart && todo == 0) {
                // byte-align: what is left of the current byte are padding bits; then RSTn
                const int real = b.bits - b.pad;
                if (real < 0 || real >= 8) return JE_BADARG;
                const uint8_t* q = b.p;
                if (q >= b.end || *q != 0xFF) return JE_BADARG;
                while (q < b.end && *q == 0xFF) q++;
                if (q >= b.end || *q != 0xD0 + next_rst) return JE_BADARG;
                b.p = q + 1;
                b.acc = 0; b.bits = 0; b.pad = 0; b.stopped = false;
                next_rst = (next_rst + 1) & 7;
                dcpred[0] = dcpred[1] = dcpred[2] = 0;
                todo = s.restart;
            }
            for (int c = 0; c < g.ncomp; c++) {
                const int h = c == 0 ? g.hl : 1, v = c == 0 ? g.vl : 1;
                const JeHuff& dct = dcs[s.td[c]];
                const JeHuff& act = acs[s.ta[c]];
                const int* cl = lim[c];
                for (int by = 0; by < v; by++) {
                    for (int bx = 0; bx < h; bx++) {
                        int16_t* blk = coef + 64 * (g.block_base[c] + (int64_t)(my * v + by) * g.bw[c] + (mx * h + bx));
                        if (b.bits < 32) je_fill(b);
                        int sym = je_symbol(b, dct);
                        if (sym < 0 || sym > 11) return JE_BADARG;
                        if (sym) dcpred[c] += je_receive_extend(b, sym);
                        if (dcpred[c] < -cl[0] || dcpred[c] > cl[0]) return JE_BADARG;
                        blk[0] = (int16_t)dcpred[c];
                        for (int k = 1; k < 64;) {
                            if (b.bits < 32) je_fill(b);
                            const int f = act.fast[je_peek(b, 10)];
                            if (f) {  // a short code and its small value in one look-up
                                k += (f >> 4) & 15;
                                if (k > 63) return JE_BADARG;
                                const int at = JE_NATURAL[k], val = f >> 8;
                                if (val < -cl[at] || val > cl[at]) return JE_BADARG;
                                blk[at] = (int16_t)val;
                                b.bits -= f & 15;
                                k++;
                                continue;
                            }
                            sym = je_symbol(b, act);
                            if (sym < 0) return JE_BADARG;
                            const int r = sym >> 4, sz = sym & 15;
                            if (sz) {
                                k += r;
                                if (k > 63) return JE_BADARG;
                                const int at = JE_NATURAL[k], val = je_receive_extend(b, sz);
                                if (val < -cl[at] || val > cl[at]) return JE_BADARG;
                                blk[at] = (int16_t)val;
                                k++;
                            } else if (r == 15) {
                                k += 16;
                            } else {
                                break;
                            }
                        }
                        if (b.bits < b.pad) return JE_BADARG;  // ran past the end of the entropy-coded data
                    }
                }
            }
            todo--;
        }
    }
    return JE_OK;
}

}  // namespace mrjpeg
#endif  // MR_JPEG_ENTROPY_HPP
