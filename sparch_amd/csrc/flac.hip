// f-3: FLAC decoding on the device, straight into the padded waveform buffer of the HD collate.
//
// The reference reads Heidelberg Digits' FLAC files with torchaudio (nonspiking_datasets.py:90).  Here the host only
// parses the metadata (dataloaders/audio.py: parse_flac) and uploads the packed file bytes of a batch; this file
// decodes channel 0 of every clip into row `row` of an (n_rows, ld) fp32 or int16 buffer, which
// sparch_fbank_padded_fwd then reads.  The format is RFC 9639; nothing here is third-party code.
//
// Frame starts are byte-aligned but only known once the previous frame is decoded, so the work is speculative:
//   flac_scan_kernel    every byte of every clip: a frame sync (0xFF 0xF8) whose header is valid, CRC-8 correct and
//                       consistent with the clip's STREAMINFO is a candidate for its frame number n; the smallest
//                       offset per (clip, n) wins (atomicMin into the clip's slot n).
//   flac_decode_kernel  one lane per slot: decode the candidate, write channel 0 at sample n * block size of the row,
//                       record where the frame ended and whether its CRC-16 matched.
//   flac_chain_kernel   one lane per clip: frame 0 must sit at the first-frame offset and every accepted frame where
//                       the previous one ended.  Where that fails (residual bytes that looked like a header), the
//                       lane decodes the frame serially from the true offset, overwriting slot n's samples, and goes
//                       on until the chain agrees again.  The frames must add up to exactly total_samples, every
//                       CRC-16 must match; otherwise the clip's first failing frame and a reason go to the error
//                       record.
// A candidate for slot n writes only inside samples [n * max_block, (n + 1) * max_block) of its row, the range the
// true frame n covers, and the chain kernel runs after every decode lane has finished: a false candidate's samples are
// always overwritten.  Variable-blocking streams (sample numbers in the headers) are decoded serially by the chain
// kernel alone.
//
// Safety: every read stays inside the clip's bytes (4-byte words of the clip's 4-aligned slot of the packed
// buffer; bits past the clip's end read as zero and make the frame fail), every write inside samples
// [0, total_samples) of the clip's row, and every loop is bounded by the clip's size, whatever the bytes say.
#include <climits>

#include "common.h"

namespace {

// per-clip table columns (SPARCH_FLAC_CLIP_FIELDS int64 per clip)
enum { C_BEGIN, C_END, C_FIRST, C_TOTAL, C_ROW, C_RATE, C_CHANNELS, C_BPS, C_MIN_BLOCK, C_MAX_BLOCK, C_SLOT_BASE,
       C_SLOTS, C_SCRATCH_BASE };
static_assert(C_SCRATCH_BASE + 1 == SPARCH_FLAC_CLIP_FIELDS, "clip table layout");

constexpr int WAVE = 64;

// one frame slot of the workspace: the winning candidate's offset (relative to the clip's begin; 0xFFFFFFFF = none)
// and what decoding it gave
struct Slot {
    uint32_t cand;
    uint32_t end;     // offset one past the frame's CRC-16
    int32_t bs;       // samples in the frame
    int32_t status;   // 0 = decoded, CRC-16 good; SPARCH_FLAC_E* otherwise; -1 = not decoded
};
static_assert(sizeof(Slot) == 16, "slot layout");

struct Clip {
    const uint8_t* bytes;   // clip's first byte (4-aligned)
    uint32_t len;           // bytes of the clip
    uint32_t first;         // first frame, relative to bytes
    long long total;        // samples per channel
    int row, rate, channels, bps, min_bs, max_bs, variable;
    long long slot_base, slots, scratch_base;
};

// A clip's table row, checked against the buffers it points into: false = SPARCH_FLAC_ETABLE for the clip.
__device__ bool load_clip(const long long* __restrict__ tab, int i, const uint8_t* bytes, long long n_bytes,
                          long long n_slots, long long n_scratch, int n_rows, int ld, int out_dtype, Clip& c) {
    const long long* t = tab + (size_t)i * SPARCH_FLAC_CLIP_FIELDS;
    const long long begin = t[C_BEGIN], end = t[C_END], first = t[C_FIRST];
    c.total = t[C_TOTAL];
    const long long row = t[C_ROW], rate = t[C_RATE], ch = t[C_CHANNELS], bps = t[C_BPS];
    const long long mn = t[C_MIN_BLOCK], mx = t[C_MAX_BLOCK];
    c.slot_base = t[C_SLOT_BASE]; c.slots = t[C_SLOTS]; c.scratch_base = t[C_SCRATCH_BASE];
    if (begin < 0 || (begin & 3) || first < begin || end <= first + 1 || end > n_bytes || end - begin >= INT_MAX)
        return false;
    if (c.total <= 0 || c.total > ld || row < 0 || row >= n_rows || rate <= 0 || rate >= (1 << 20) || ch < 1 ||
        ch > 8 || bps < 4 || bps > 24 || (out_dtype == 1 && bps != 16) || mn < 1 || mn > mx || mx > 65535)
        return false;
    if (c.slots < 1 || c.slot_base < 0 || c.slot_base > n_slots - c.slots) return false;
    if (ch == 2 && (c.scratch_base < 0 || c.slots > (n_scratch - c.scratch_base) / mx)) return false;
    c.bytes = bytes + begin;
    c.len = (uint32_t)(end - begin);
    c.first = (uint32_t)(first - begin);
    c.row = (int)row; c.rate = (int)rate; c.channels = (int)ch; c.bps = (int)bps; c.min_bs = (int)mn;
    c.max_bs = (int)mx;
    c.variable = c.bytes[c.first + 1] & 1;  // blocking strategy of the first frame (0xF8 fixed, 0xF9 variable)
    return true;
}

__device__ __forceinline__ int byte_at(const Clip& c, uint32_t off) { return off < c.len ? (int)c.bytes[off] : -1; }

__device__ uint32_t crc8(const Clip& c, uint32_t off, uint32_t n) {  // poly 0x07, init 0 (headers: <= 15 bytes)
    uint32_t crc = 0;
    for (uint32_t k = 0; k < n; ++k) {
        crc ^= c.bytes[off + k];
        for (int b = 0; b < 8; ++b) crc = (crc & 0x80) ? ((crc << 1) ^ 0x07) & 0xFF : (crc << 1) & 0xFF;
    }
    return crc;
}

struct Header {
    int bs, assign, len;
    long long number;  // frame number (fixed blocking) or first sample (variable)
};

// The frame header at `off`, checked field by field, by its CRC-8 and against the clip's STREAMINFO (blocking
// strategy, channels, bits per sample, sample rate when coded, block size <= max_block).
__device__ bool parse_header(const Clip& c, uint32_t off, Header& h) {
    const int b0 = byte_at(c, off), b1 = byte_at(c, off + 1), b2 = byte_at(c, off + 2), b3 = byte_at(c, off + 3);
    if (b0 != 0xFF || b1 < 0 || (b1 & 0xFE) != 0xF8 || (b1 & 1) != c.variable || b2 < 0 || b3 < 0) return false;
    const int bs_code = b2 >> 4, sr_code = b2 & 15, assign = b3 >> 4, ss_code = (b3 >> 1) & 7;
    if (bs_code == 0 || sr_code == 15 || assign > 10 || ss_code == 3 || ss_code == 7 || (b3 & 1)) return false;
    if ((assign < 8 ? assign + 1 : 2) != c.channels) return false;
    if (ss_code != 0) {
        const int ss_bits[8] = {0, 8, 12, 0, 16, 20, 24, 0};
        if (ss_bits[ss_code] != c.bps) return false;
    }
    uint32_t p = off + 4;
    int x = byte_at(c, p++);
    if (x < 0) return false;
    int extra;
    long long v;
    if (!(x & 0x80)) { v = x; extra = 0; }
    else if ((x & 0xE0) == 0xC0) { v = x & 0x1F; extra = 1; }
    else if ((x & 0xF0) == 0xE0) { v = x & 0x0F; extra = 2; }
    else if ((x & 0xF8) == 0xF0) { v = x & 0x07; extra = 3; }
    else if ((x & 0xFC) == 0xF8) { v = x & 0x03; extra = 4; }
    else if ((x & 0xFE) == 0xFC) { v = x & 0x01; extra = 5; }
    else if (x == 0xFE) { v = 0; extra = 6; }
    else return false;
    if (!c.variable && extra > 5) return false;  // frame numbers have at most 31 bits
    for (int k = 0; k < extra; ++k) {
        const int y = byte_at(c, p++);
        if (y < 0 || (y & 0xC0) != 0x80) return false;
        v = (v << 6) | (y & 0x3F);
    }
    int bs;
    if (bs_code == 1) bs = 192;
    else if (bs_code <= 5) bs = 576 << (bs_code - 2);
    else if (bs_code == 6) { const int y = byte_at(c, p++); if (y < 0) return false; bs = y + 1; }
    else if (bs_code == 7) {
        const int y0 = byte_at(c, p), y1 = byte_at(c, p + 1);
        if (y0 < 0 || y1 < 0) return false;
        bs = ((y0 << 8) | y1) + 1;
        p += 2;
    } else bs = 256 << (bs_code - 8);
    if (sr_code != 0) {
        const int rates[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
        int rate;
        if (sr_code < 12) rate = rates[sr_code];
        else if (sr_code == 12) { const int y = byte_at(c, p++); if (y < 0) return false; rate = y * 1000; }
        else {
            const int y0 = byte_at(c, p), y1 = byte_at(c, p + 1);
            if (y0 < 0 || y1 < 0) return false;
            rate = ((y0 << 8) | y1) * (sr_code == 14 ? 10 : 1);
            p += 2;
        }
        if (rate != c.rate) return false;
    }
    const int crc = byte_at(c, p);
    if (crc < 0 || (uint32_t)crc != crc8(c, off, p - off)) return false;
    if (bs > c.max_bs) return false;
    h.bs = bs; h.assign = assign; h.len = (int)(p + 1 - off); h.number = v;
    return true;
}

// First sample of a frame and whether its size fits the stream: a fixed-blocking frame n starts at n * max_block
// and is max_block long unless it is the last; a variable-blocking frame is at least min_block long unless it is the
// last.  Nothing may run past total_samples.
__device__ bool frame_span(const Clip& c, const Header& h, long long& first) {
    first = c.variable ? h.number : h.number * c.max_bs;
    if (first < 0 || first >= c.total || h.bs > c.total - first) return false;
    const bool last = first + h.bs == c.total;
    return last || (c.variable ? h.bs >= c.min_bs : h.bs == c.max_bs);
}

// MSB-first bit reader over a clip's bytes, refilled from aligned 32-bit words into a left-aligned 64-bit buffer.
// Words past the clip read as zero; a frame whose bits run past the clip's end is caught by overrun().
struct Bits {
    const uint32_t* w;
    uint32_t nwords, len_bits, next;
    uint64_t buf;
    int nbuf;

    __device__ void init(const Clip& c, uint32_t off) {
        w = reinterpret_cast<const uint32_t*>(c.bytes);
        nwords = (c.len + 3) >> 2;
        len_bits = c.len * 8u;
        next = off >> 2; buf = 0; nbuf = 0;
        refill();
        skip((off & 3) * 8);
    }
    __device__ __forceinline__ void refill() {
        while (nbuf <= 32) {
            const uint32_t v = next < nwords ? __builtin_bswap32(w[next]) : 0u;
            ++next;
            buf |= (uint64_t)v << (32 - nbuf);
            nbuf += 32;
        }
    }
    __device__ __forceinline__ uint32_t get(int n) {  // 0 <= n <= 32
        if (n == 0) return 0;
        if (nbuf < n) refill();
        const uint32_t v = (uint32_t)(buf >> (64 - n));
        buf <<= n;
        nbuf -= n;
        return v;
    }
    __device__ __forceinline__ int32_t get_signed(int n) {  // 1 <= n <= 32
        const uint32_t v = get(n);
        return n == 32 ? (int32_t)v : (int32_t)(v << (32 - n)) >> (32 - n);
    }
    __device__ __forceinline__ void skip(int n) {
        while (n > 32) { get(32); n -= 32; }
        get(n);
    }
    __device__ __forceinline__ long long pos() const { return (long long)next * 32 - nbuf; }  // bits consumed
    __device__ __forceinline__ bool overrun() const { return pos() > (long long)len_bits; }
    // number of 0 bits before the next 1 (the 1 is consumed); stops once past the clip's end
    __device__ __forceinline__ uint32_t unary() {
        uint32_t q = 0;
        for (;;) {
            if (nbuf == 0) refill();
            if (buf != 0) {
                const int z = __builtin_clzll(buf);
                buf <<= z; buf <<= 1;
                nbuf -= z + 1;
                return q + (uint32_t)z;
            }
            q += (uint32_t)nbuf;
            nbuf = 0;
            if (overrun()) return q;
        }
    }
};

// where a decoded subframe's samples go (after the wasted-bits shift)
enum Sink { TO_OUT, TO_SCRATCH, DROP, RIGHT_SIDE, MID_SIDE };

struct Target {
    void* out;           // the clip's row, starting at the frame's first sample
    int32_t* scratch;    // max_block int32 for the first subframe of a decorrelated pair (nullptr for mono)
    long long room;      // samples of the row the frame may write: total_samples - first
    float scale;         // 2^-(bps - 1)
    int dtype;           // 0 fp32, 1 int16
};

__device__ __forceinline__ void emit(const Target& t, int mode, int i, int32_t x) {
    if (mode == DROP) return;
    if (mode == TO_SCRATCH) { t.scratch[i] = x; return; }
    int32_t left = x;
    if (mode == RIGHT_SIDE) left = t.scratch[i] + x;          // side (subframe 0) + right
    else if (mode == MID_SIDE) {                              // mid (subframe 0), side (x)
        const int32_t mid = (int32_t)(((uint32_t)t.scratch[i] << 1) | (uint32_t)(x & 1));
        left = (int32_t)(((int64_t)mid + x) >> 1);
    }
    if (i >= t.room) return;
    if (t.dtype == 1) static_cast<int16_t*>(t.out)[i] = (int16_t)left;
    else static_cast<float*>(t.out)[i] = (float)left * t.scale;
}

// Prediction over the N most recent samples, kept in registers (h[0] newest); coefficients past the predictor's
// order are 0, so orders up to N share one code path.  `warm` holds the subframe's first `order` samples (read by
// the caller), the partitioned residual follows in the stream.
template <int N>
__device__ int predict(Bits& br, const Target& t, int mode, const int32_t* coef, const int32_t* warm, int order,
                       int shift, int k, int bs) {
    int32_t c[N], h[N];
#pragma unroll
    for (int j = 0; j < N; ++j) { c[j] = j < order ? coef[j] : 0; h[j] = 0; }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (i < order) {
#pragma unroll
            for (int j = N - 1; j > 0; --j) h[j] = h[j - 1];
            h[0] = warm[i];
            emit(t, mode, i, (int32_t)((uint32_t)warm[i] << k));
        }
    }
    const uint32_t method = br.get(2);
    if (method > 1) return SPARCH_FLAC_ESUBFRAME;
    const int pbits = method ? 5 : 4, escape = method ? 31 : 15;
    const int porder = (int)br.get(4);
    const int part = bs >> porder;
    if ((part << porder) != bs || part < order) return SPARCH_FLAC_ESUBFRAME;
    int i = order;
    for (int p = 0; p < (1 << porder); ++p) {     // partition 0 holds part - order residuals
        const int param = (int)br.get(pbits);
        const int raw = param == escape ? (int)br.get(5) : -1;  // escaped: residuals of `raw` bits each
        if (br.overrun()) return SPARCH_FLAC_ETRUNC;
        for (const int end = (p + 1) * part; i < end; ++i) {
            int32_t r;
            if (raw < 0) {
                const uint32_t q = br.unary();
                const uint32_t u = (q << param) | br.get(param);
                r = (int32_t)(u >> 1) ^ -(int32_t)(u & 1);
            } else {
                r = raw ? br.get_signed(raw) : 0;
            }
            long long acc = 0;
#pragma unroll
            for (int j = 0; j < N; ++j) acc += (long long)c[j] * h[j];
            const int32_t v = (int32_t)((uint32_t)r + (uint32_t)(int32_t)(acc >> shift));
#pragma unroll
            for (int j = N - 1; j > 0; --j) h[j] = h[j - 1];
            h[0] = v;
            emit(t, mode, i, (int32_t)((uint32_t)v << k));
            if (br.overrun()) return SPARCH_FLAC_ETRUNC;
        }
    }
    return 0;
}

// One subframe of `bps` bits (the side channel of a decorrelated pair has one more) and `bs` samples.
__device__ int subframe(Bits& br, const Target& t, int mode, int bps, int bs) {
    if (br.get(1) != 0) return SPARCH_FLAC_ESUBFRAME;
    const int type = (int)br.get(6);
    int k = 0;
    if (br.get(1)) {                                   // wasted bits: k - 1 zeros, then a one
        k = (int)br.unary() + 1;
        if (k >= bps) return SPARCH_FLAC_ESUBFRAME;
    }
    const int b = bps - k;
    if (br.overrun()) return SPARCH_FLAC_ETRUNC;
    if (type == 0) {                                   // constant
        const int32_t v = (int32_t)((uint32_t)br.get_signed(b) << k);
        for (int i = 0; i < bs; ++i) emit(t, mode, i, v);
        return br.overrun() ? SPARCH_FLAC_ETRUNC : 0;
    }
    if (type == 1) {                                   // verbatim
        for (int i = 0; i < bs; ++i) {
            emit(t, mode, i, (int32_t)((uint32_t)br.get_signed(b) << k));
            if (br.overrun()) return SPARCH_FLAC_ETRUNC;
        }
        return 0;
    }
    int order, shift = 0;
    if (type >= 8 && type <= 12) order = type - 8;     // fixed predictors of order 0-4
    else if (type >= 32) order = type - 31;            // LPC of order 1-32
    else return SPARCH_FLAC_ESUBFRAME;                 // reserved types
    if (order > bs) return SPARCH_FLAC_ESUBFRAME;
    int32_t warm[32], coef[32];
    for (int i = 0; i < order; ++i) warm[i] = br.get_signed(b);
    if (type < 32) {
        constexpr int32_t fixed[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
        for (int j = 0; j < 4; ++j) coef[j] = fixed[order][j];
    } else {
        const int prec = (int)br.get(4) + 1;           // 15 (precision 16) is invalid
        if (prec == 16) return SPARCH_FLAC_ESUBFRAME;
        shift = br.get_signed(5);
        if (shift < 0) return SPARCH_FLAC_ESUBFRAME;
        for (int i = 0; i < order; ++i) coef[i] = br.get_signed(prec);
    }
    if (br.overrun()) return SPARCH_FLAC_ETRUNC;
    if (order <= 8) return predict<8>(br, t, mode, coef, warm, order, shift, k, bs);
    if (order <= 16) return predict<16>(br, t, mode, coef, warm, order, shift, k, bs);
    return predict<32>(br, t, mode, coef, warm, order, shift, k, bs);
}

// CRC-16 (poly 0x8005, init 0, MSB first) of bytes [off, end) of the clip, through a 256-entry LDS table.
__device__ uint32_t crc16(const Clip& c, const uint16_t* tab, uint32_t off, uint32_t end) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(c.bytes);
    uint32_t crc = 0;
    for (uint32_t q = off >> 2; q * 4 < end; ++q) {
        const uint32_t word = w[q];
        const uint32_t lo = q * 4 < off ? off - q * 4 : 0, hi = min(4u, end - q * 4);
        for (uint32_t b = lo; b < hi; ++b)
            crc = ((crc << 8) ^ tab[((crc >> 8) ^ (word >> (8 * b))) & 0xFF]) & 0xFFFF;
    }
    return crc;
}

__device__ void crc16_table(uint16_t* tab) {
    for (int v = threadIdx.x; v < 256; v += blockDim.x) {
        uint32_t r = (uint32_t)v << 8;
        for (int b = 0; b < 8; ++b) r = (r & 0x8000) ? (r << 1) ^ 0x8005 : r << 1;
        tab[v] = (uint16_t)r;
    }
    __syncthreads();
}

struct Decoded {
    uint32_t end;
    int bs, status;
};

// Decode the frame at `off` whose header must carry `number` (frame number, or first sample when variable): channel
// 0 into the clip's row, the first subframe of a decorrelated pair into `scratch`.
__device__ Decoded decode_frame(const Clip& c, const uint16_t* crc_tab, uint32_t off, long long number, void* out,
                                int ld, int dtype, int32_t* scratch) {
    Decoded d{0, 0, SPARCH_FLAC_EHEADER};
    Header h;
    long long first;
    if (!parse_header(c, off, h) || h.number != number || !frame_span(c, h, first)) return d;
    d.bs = h.bs;
    Target t;
    t.room = c.total - first;
    t.scale = __int_as_float((127 - (c.bps - 1)) << 23);
    t.dtype = dtype;
    t.scratch = scratch;
    t.out = dtype == 1 ? (void*)(static_cast<int16_t*>(out) + (size_t)c.row * ld + first)
                       : (void*)(static_cast<float*>(out) + (size_t)c.row * ld + first);
    Bits br;
    br.init(c, off + (uint32_t)h.len);
    for (int ch = 0; ch < c.channels; ++ch) {
        int mode = ch == 0 ? TO_OUT : DROP, bps = c.bps;
        if (h.assign == 8) bps += ch;                                   // left, side
        else if (h.assign == 9) { bps += 1 - ch; mode = ch ? RIGHT_SIDE : TO_SCRATCH; }   // side, right
        else if (h.assign == 10) { bps += ch; mode = ch ? MID_SIDE : TO_SCRATCH; }       // mid, side
        const int s = subframe(br, t, mode, bps, h.bs);
        if (s) { d.status = s; return d; }
    }
    br.skip((int)((8 - (br.pos() & 7)) & 7));                         // zero padding to a byte
    const long long crc_pos = br.pos() >> 3;
    const uint32_t stored = br.get(16);
    if (br.overrun()) { d.status = SPARCH_FLAC_ETRUNC; return d; }
    d.end = (uint32_t)(crc_pos + 2);
    d.status = crc16(c, crc_tab, off, (uint32_t)crc_pos) == stored ? 0 : SPARCH_FLAC_ECRC;
    return d;
}

__device__ __forceinline__ int32_t* slot_scratch(const Clip& c, int32_t* scratch, long long n) {
    return c.channels == 2 ? scratch + c.scratch_base + n * c.max_bs : nullptr;
}

struct Args {
    const long long* clips;
    const uint8_t* bytes;
    long long n_bytes, n_slots, n_scratch;
    int n_clips, n_rows, ld, dtype;
    void* out;
    long long* err;
    Slot* slots;
    int32_t* scratch;
};

__device__ __forceinline__ bool clip_of(const Args& a, int i, Clip& c) {
    return load_clip(a.clips, i, a.bytes, a.n_bytes, a.n_slots, a.n_scratch, a.n_rows, a.ld, a.dtype, c);
}

// grid (x, n_clips): the blocks of clip y stride over its 4-byte words from the first frame on
__global__ void __launch_bounds__(256) flac_scan_kernel(Args a) {
    Clip c;
    if (!clip_of(a, blockIdx.y, c) || c.variable) return;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(c.bytes);
    const uint32_t nwords = (c.len + 3) >> 2;
    for (uint32_t q = (c.first >> 2) + blockIdx.x * blockDim.x + threadIdx.x; q < nwords;
         q += gridDim.x * blockDim.x) {
        const uint32_t word = w[q], nxt = q + 1 < nwords ? w[q + 1] : 0u;
        for (int b = 0; b < 4; ++b) {
            const uint32_t off = q * 4 + b;
            const uint32_t b0 = (word >> (8 * b)) & 0xFF, b1 = b < 3 ? (word >> (8 * b + 8)) & 0xFF : nxt & 0xFF;
            if (b0 != 0xFF || b1 != 0xF8 || off < c.first || off + 1 >= c.len) continue;
            Header h;
            long long first;
            if (!parse_header(c, off, h) || h.number >= c.slots || !frame_span(c, h, first)) continue;
            atomicMin(&a.slots[c.slot_base + h.number].cand, off);
        }
    }
}

// grid cdiv(n_slots, 64) x 64: lane = slot; the slot's clip by binary search over the table's slot bases
__global__ void __launch_bounds__(WAVE) flac_decode_kernel(Args a) {
    __shared__ uint16_t tab[256];
    crc16_table(tab);
    const long long s = (long long)blockIdx.x * WAVE + threadIdx.x;
    if (s >= a.n_slots) return;
    const uint32_t cand = a.slots[s].cand;
    if (cand == 0xFFFFFFFFu) return;
    int lo = 0, hi = a.n_clips - 1;                 // last clip whose slot base is <= s
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.clips[(size_t)mid * SPARCH_FLAC_CLIP_FIELDS + C_SLOT_BASE] <= s) lo = mid; else hi = mid - 1;
    }
    Clip c;
    if (!clip_of(a, lo, c) || c.variable || s < c.slot_base || s >= c.slot_base + c.slots) return;
    const long long n = s - c.slot_base;
    const Decoded d = decode_frame(c, tab, cand, n, a.out, a.ld, a.dtype, slot_scratch(c, a.scratch, n));
    a.slots[s].end = d.end;
    a.slots[s].bs = d.bs;
    a.slots[s].status = d.status;
}

__device__ void flac_fail(long long* err, int clip, long long frame, int reason) {
    atomicAdd(reinterpret_cast<unsigned long long*>(err), 1ull);
    const unsigned long long key = ((unsigned long long)clip << 32) |
                                   ((unsigned long long)min(frame, 0xFFFFFFll) << 8) | (unsigned long long)reason;
    atomicMin(reinterpret_cast<unsigned long long*>(err + 1), key);
}

// grid cdiv(n_clips, 64) x 64: lane = clip
__global__ void __launch_bounds__(WAVE) flac_chain_kernel(Args a) {
    __shared__ uint16_t tab[256];
    crc16_table(tab);
    const int i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= a.n_clips) return;
    Clip c;
    if (!clip_of(a, i, c)) { flac_fail(a.err, i, 0, SPARCH_FLAC_ETABLE); return; }
    uint32_t off = c.first;
    long long done = 0, n = 0;
    for (; done < c.total && n < c.slots; ++n) {
        const Slot sl = a.slots[c.slot_base + n];
        if (!c.variable && sl.cand == off && sl.status == 0) { done += sl.bs; off = sl.end; continue; }
        const Decoded d = decode_frame(c, tab, off, c.variable ? done : n, a.out, a.ld, a.dtype,
                                       slot_scratch(c, a.scratch, n));
        if (d.status) { flac_fail(a.err, i, n, d.status); return; }
        done += d.bs;
        off = d.end;
    }
    if (done != c.total) flac_fail(a.err, i, n, SPARCH_FLAC_ELENGTH);
}

}  // namespace

extern "C" size_t sparch_flac_workspace_bytes(long long n_slots, long long n_scratch) {
    SPARCH_ENTER();
    if (n_slots <= 0 || n_slots > INT_MAX || n_scratch < 0 || n_scratch > (1ll << 40)) return 0;
    return (((size_t)n_slots * sizeof(Slot) + 255) & ~(size_t)255) + (size_t)n_scratch * sizeof(int32_t);
}

extern "C" int sparch_flac_decode_padded(int n_clips, const long long* clips, const unsigned char* bytes,
                                         long long n_bytes, long long n_slots, long long n_scratch, int n_rows, int ld,
                                         int out_dtype, void* out, long long* err, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    SPARCH_ENTER();
    if (n_clips <= 0 || n_clips > 65535 || !clips || !bytes || n_bytes <= 0 || n_rows <= 0 || ld <= 0 ||
        (out_dtype != 0 && out_dtype != 1) || !out || !err || !workspace)
        return SPARCH_EINVAL;
    const size_t need = sparch_flac_workspace_bytes(n_slots, n_scratch);
    if (need == 0) return SPARCH_EINVAL;
    if ((n_bytes & 3) || (reinterpret_cast<uintptr_t>(bytes) & 3) || !aligned16(workspace) ||
        (reinterpret_cast<uintptr_t>(err) & 7))
        return SPARCH_EALIGN;
    if (workspace_bytes < need) return SPARCH_EWORKSPACE;
    Args a;
    a.clips = clips; a.bytes = bytes; a.n_bytes = n_bytes; a.n_slots = n_slots; a.n_scratch = n_scratch;
    a.n_clips = n_clips; a.n_rows = n_rows; a.ld = ld; a.dtype = out_dtype; a.out = out; a.err = err;
    a.slots = static_cast<Slot*>(workspace);
    a.scratch = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + (need - (size_t)n_scratch * 4));
    hipStream_t st = (hipStream_t)stream;
    // error record: no clip in error, key all ones (atomicMin); every slot: no candidate, not decoded
    hipError_t e = hipMemsetAsync(err, 0, sizeof(long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(err + 1, 0xFF, sizeof(long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(a.slots, 0xFF, (size_t)n_slots * sizeof(Slot), st);
    if (e != hipSuccess) { sparch_note_hip_error((int)e); return SPARCH_ELAUNCH; }
    // scan: ~4 KiB of bytes per block on average over the clips, at most 64 blocks per clip
    const long long per_clip = n_bytes / n_clips;
    const unsigned gx = (unsigned)(per_clip / 4096 + 1 < 64 ? per_clip / 4096 + 1 : 64);
    hipLaunchKernelGGL(flac_scan_kernel, dim3(gx, (unsigned)n_clips), dim3(256), 0, st, a);
    SPARCH_CHECK_LAUNCH();
    hipLaunchKernelGGL(flac_decode_kernel, dim3((unsigned)((n_slots + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, a);
    SPARCH_CHECK_LAUNCH();
    hipLaunchKernelGGL(flac_chain_kernel, dim3((unsigned)cdiv(n_clips, WAVE)), dim3(WAVE), 0, st, a);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}
