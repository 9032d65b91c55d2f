// gm_inflate.inc -- the gzip request parser (SURVEY.md §8 f4, Wallarm's `gzip` parser), included
// into gm_device.hip's anonymous namespace: an RFC 1951 inflate of the first RFC 1952 member of a
// request body, one wave (64 lanes) per stream.
//
// A body is a gzip member if it starts 1f 8b 08, the reserved FLG bits are zero and it is at least
// 18 bytes long -- recognised by its bytes, not by a Content-Encoding header (the attacker's to
// choose).  FEXTRA / FNAME / FCOMMENT / FHCRC are skipped, bounded by the body.  The trailer's
// ISIZE sizes the output in O(1): request i gets a slot of
//     L = min(ISIZE, GM_INFLATE_RATIO * body_len, GM_INFLATE_MAX)
// bytes (one exclusive scan over the batch), so the batch needs at most GM_INFLATE_RATIO *
// arena_len bytes whatever the bodies claim.  A stream longer than L is cut at L (its prefix is the
// view); a stream that ends with another size than ISIZE, or any malformed block, is corrupt: no
// view, length GM_NONE.  CRC-32 is NOT verified: scanning a body the backend would refuse costs a
// scan and nothing else.  Only the first member is inflated.
//
// Work split: k_infl_size (a lane per request) compacts the gzip bodies' indices into a list;
// k_inflate's persistent 256-thread workgroups pull from it, a wave owning a stream from its first
// bit to its last.  Per wave ~4.3 KiB of LDS (InflLds): a 2^10-entry primary table for the
// literal/length code, 2^9 for the distance code (symbol | length << 9, u16), and the canonical
// first-code / count / sorted-symbol arrays that decode the longer codes.
//
// The bit reader is wave-uniform (bit buffer, bit count and position are the same in every lane,
// i.e. scalar registers): lane l holds dword l of the current 256-byte chunk of the body, loaded
// through a buffer resource over the body (a read past it returns 0 and touches nothing), the next
// chunk is already in flight, and a refill is one v_readlane.  Tokens are decoded serially, up to
// 64 at a time into one VGPR (token k in lane k, a compare and select), then resolved by all lanes: a wave
// prefix sum of the token lengths places them, literals are stored one per lane, matches are
// copied wave-wide in token order out of the output itself (the window), the source index folded
// modulo the distance when dist < len so that only bytes before the match are read.  Every write
// to memory is a vector store.

#ifndef GM_INFLATE_RATIO
#define GM_INFLATE_RATIO 8
#endif
#ifndef GM_INFLATE_MAX
#define GM_INFLATE_MAX (1u << 20)
#endif
constexpr uint32_t INFL_BLOCK = 256, INFL_WAVES = INFL_BLOCK / 64;
constexpr uint32_t INFL_LBITS = 10, INFL_DBITS = 9, INFL_CBITS = 7;
constexpr uint32_t INFL_NLIT = 288, INFL_NDIST = 32;
// control words of one launch: [0] gzip bodies listed, [1] the list's queue head, [2] views given
constexpr uint32_t INFL_CTL_WORDS = 4;
constexpr uint32_t INFL_VIEWS_WORD = 24;                        // batch status word: bodies given a view
constexpr uint32_t INFL_STATUS_WORD = UPURI_STATUS_WORD + 1;    // gm_inflate_bodies: output capacity exceeded

struct InflLds {                       // one wave's decode tables
    uint16_t lit[1u << INFL_LBITS];    // primary: symbol | length << 9, 0 = a longer (or no) code
    uint16_t dist[1u << INFL_DBITS];   // (holds the code-length code's table while lengths are read)
    uint16_t sorted[2][INFL_NLIT];     // symbols by (code length, symbol): [0] lit/len, [1] distance
    uint16_t first[2][16], count[2][16], offs[2][16];   // canonical code of each length
    uint32_t cnt[16];
    uint8_t lens[INFL_NLIT + INFL_NDIST];
};
static_assert(sizeof(InflLds) * INFL_WAVES <= 20 * 1024, "8 inflate workgroups per CU");

__device__ __forceinline__ uint32_t infl_u(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
// the wave's LDS writes before its reads of other lanes' entries (one wave: no s_barrier)
__device__ __forceinline__ void infl_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// the wave's global stores before its later loads of the same bytes
__device__ __forceinline__ void infl_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ __forceinline__ uint32_t infl_limit(uint32_t isize, uint32_t body_len) {
    const uint64_t r = (uint64_t)GM_INFLATE_RATIO * body_len;
    return (uint32_t)min((uint64_t)min(isize, (uint32_t)GM_INFLATE_MAX), r);
}
__device__ __forceinline__ bool infl_is_member(const uint8_t *b, uint32_t n) {
    return n >= 18 && b[0] == 0x1f && b[1] == 0x8b && b[2] == 8 && !(b[3] & 0xE0);
}
__device__ __forceinline__ uint32_t infl_isize(const uint8_t *b, uint32_t n) {
    return (uint32_t)b[n - 4] | (uint32_t)b[n - 3] << 8 | (uint32_t)b[n - 2] << 16 | (uint32_t)b[n - 1] << 24;
}

// ---- the wave-uniform bit reader
struct InflIn {
    __amdgpu_buffer_rsrc_t rs;   // the body from its dword-aligned start
    uint32_t cur, nxt;           // lane l: dword l of the current / the next 256-byte chunk
    uint32_t dw;                 // the next dword to take
    uint64_t bb;                 // bit buffer, LSB first
    uint32_t bc;                 // its valid bits
    uint32_t lane;
};
__device__ __forceinline__ uint32_t infl_take(InflIn &in) {
    const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)in.cur, (int)(in.dw & 63));
    in.dw++;
    if ((in.dw & 63) == 0) {
        in.cur = in.nxt;
        in.nxt = __builtin_amdgcn_raw_buffer_load_b32(in.rs, (in.dw + 64 + in.lane) * 4, 0, 0);
    }
    return w;
}
// position the reader at byte p of the resource
__device__ __forceinline__ void infl_seek(InflIn &in, uint32_t p) {
    in.dw = p >> 2;
    const uint32_t c0 = in.dw & ~63u;
    in.cur = __builtin_amdgcn_raw_buffer_load_b32(in.rs, (c0 + in.lane) * 4, 0, 0);
    in.nxt = __builtin_amdgcn_raw_buffer_load_b32(in.rs, (c0 + 64 + in.lane) * 4, 0, 0);
    const uint32_t sh = (p & 3) * 8;
    in.bb = infl_take(in) >> sh;
    in.bc = 32 - sh;
}
// at least 32 valid bits
__device__ __forceinline__ void infl_refill(InflIn &in) {
    if (in.bc < 32) {
        in.bb |= (uint64_t)infl_take(in) << in.bc;
        in.bc += 32;
    }
}
__device__ __forceinline__ uint32_t infl_bits(InflIn &in, uint32_t n) {
    const uint32_t v = (uint32_t)in.bb & ((1u << n) - 1);
    in.bb >>= n;
    in.bc -= n;
    return v;
}
__device__ __forceinline__ uint64_t infl_bitpos(const InflIn &in) { return (uint64_t)in.dw * 32 - in.bc; }

// ---- canonical Huffman tables from code lengths, wave-parallel.  lens[0, n) -> the primary table
// tab (2^pbits entries) and slot's first / count / offs / sorted arrays.  kind: 0 lit/len,
// 1 distance, 2 the code-length code.  Over-subscribed sets are rejected, incomplete ones too but
// for what zlib allows: no code at all, or one code of length 1 (never for the code-length code).
__device__ bool infl_build(InflLds &W, const uint8_t *lens, uint32_t n, uint16_t *tab, uint32_t pbits,
                           uint32_t slot, uint32_t kind, uint32_t lane) {
    uint32_t *tab32 = reinterpret_cast<uint32_t *>(tab);
    for (uint32_t i = lane; i < (1u << pbits) / 2; i += 64) tab32[i] = 0;
    if (lane < 16) W.cnt[lane] = 0;
    infl_sync();
    for (uint32_t s = lane; s < n; s += 64) {
        const uint32_t l = lens[s];
        if (l) atomicAdd(&W.cnt[l], 1u);
    }
    infl_sync();
    uint32_t code = 0, total = 0, prev = 0, maxl = 0;
    int left = 1;
    bool over = false;
    for (uint32_t l = 1; l <= 15; l++) {
        const uint32_t k = infl_u(W.cnt[l]);
        code = (code + prev) << 1;
        left = (left << 1) - (int)k;
        over |= left < 0;
        if (lane == 0) { W.first[slot][l] = (uint16_t)code; W.count[slot][l] = (uint16_t)k; W.offs[slot][l] = (uint16_t)total; }
        total += k;
        prev = k;
        if (k) maxl = l;
    }
    if (over) return false;
    if (left > 0 && (kind == 2 || (total != 0 && maxl != 1))) return false;
    infl_sync();
    // each lane owns the symbols lane, lane + 64, ...: its rank among the symbols of its length
    // (ballots, in symbol order) gives the code; the entry is replicated over the primary table
    uint32_t base[16];
#pragma unroll
    for (uint32_t b = 0; b < 16; b++) base[b] = 0;
    for (uint32_t s0 = 0; s0 < n; s0 += 64) {
        const uint32_t s = s0 + lane;
        const uint32_t l = s < n ? lens[s] : 0u;
        uint32_t rank = 0;
#pragma unroll
        for (uint32_t b = 1; b <= 15; b++) {
            const unsigned long long m = __ballot(l == b);
            if (l == b) rank = base[b] + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            base[b] += (uint32_t)__popcll(m);
        }
        if (l) {
            const uint32_t c = (uint32_t)W.first[slot][l] + rank;
            W.sorted[slot][(uint32_t)W.offs[slot][l] + rank] = (uint16_t)s;
            if (l <= pbits) {
                const uint16_t e = (uint16_t)(s | l << 9);
                for (uint32_t k = __brev(c) >> (32 - l); k < (1u << pbits); k += 1u << l) tab[k] = e;
            }
        }
    }
    infl_sync();
    return true;
}

// one symbol of the code in (tab, slot): the primary table, then the canonical arrays for a code
// longer than pbits.  false: no such code.  (At least 15 valid bits in the buffer.)
__device__ __forceinline__ bool infl_sym(const InflLds &W, InflIn &in, const uint16_t *tab, uint32_t pbits, uint32_t slot,
                                         uint32_t &sym) {
    const uint32_t e = infl_u(tab[(uint32_t)in.bb & ((1u << pbits) - 1)]);
    if (e) {
        sym = e & 511;
        infl_bits(in, e >> 9);
        return true;
    }
    uint32_t code = __brev((uint32_t)in.bb & ((1u << pbits) - 1)) >> (32 - pbits);
    for (uint32_t l = pbits + 1; l <= 15; l++) {
        code = code << 1 | ((uint32_t)(in.bb >> (l - 1)) & 1);
        const uint32_t k = code - infl_u(W.first[slot][l]);
        if (k < infl_u(W.count[slot][l])) {
            sym = infl_u(W.sorted[slot][infl_u(W.offs[slot][l]) + k]);
            infl_bits(in, l);
            return true;
        }
    }
    return false;
}

__device__ __forceinline__ uint32_t infl_scan_incl(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// a dynamic block's header: the code-length code, the two codes' lengths, their tables
__device__ bool infl_dynamic(InflLds &W, InflIn &in, uint64_t endbit, uint32_t lane) {
    // the order the code-length code's lengths come in (RFC 1951 3.2.7), 5 bits each, by lane
    const uint32_t order = lane < 6 ? (0x0E804A30u >> (5 * lane)) & 31           // 16 17 18 0 8 7
                         : lane < 12 ? (0x08B2A8C9u >> (5 * (lane - 6))) & 31    // 9 6 10 5 11 4
                         : lane < 18 ? (0x02E1346Cu >> (5 * (lane - 12))) & 31   // 12 3 13 2 14 1
                                     : 15u;
    infl_refill(in);
    const uint32_t hlit = infl_bits(in, 5) + 257, hdist = infl_bits(in, 5) + 1, hclen = infl_bits(in, 4) + 4;
    if (hlit > 286 || hdist > 30) return false;
    if (lane < 19) W.lens[lane] = 0;
    infl_sync();
    // per-lane bit-field extracts: lanes 0..9 from the first 30 bits, 10..18 from the next 27
    infl_refill(in);
    const uint32_t n1 = min(hclen, 10u);
    if (lane < n1) W.lens[order] = (uint8_t)((in.bb >> (3 * lane)) & 7);
    infl_bits(in, 3 * n1);
    infl_refill(in);
    if (lane >= 10 && lane < hclen) W.lens[order] = (uint8_t)((in.bb >> (3 * ((lane - 10) & 15))) & 7);
    infl_bits(in, 3 * (hclen - n1));
    infl_sync();
    if (!infl_build(W, W.lens, 19, W.dist, INFL_CBITS, 1, 2, lane)) return false;
    const uint32_t total = hlit + hdist;
    uint32_t i = 0, prev = 0;
    while (i < total) {
        infl_refill(in);
        uint32_t s;
        if (!infl_sym(W, in, W.dist, INFL_CBITS, 1, s)) return false;
        uint32_t rep = 1, val = s;
        if (s < 16) prev = s;
        else if (s == 16) { if (i == 0) return false; val = prev; rep = 3 + infl_bits(in, 2); }
        else if (s == 17) { val = prev = 0; rep = 3 + infl_bits(in, 3); }
        else { val = prev = 0; rep = 11 + infl_bits(in, 7); }
        if (i + rep > total || infl_bitpos(in) > endbit) return false;
        for (uint32_t j = lane; j < rep; j += 64) W.lens[i + j] = (uint8_t)val;
        i += rep;
    }
    infl_sync();
    if (infl_u(W.lens[256]) == 0) return false;   // no end-of-block code
    // (the distance lengths follow the lit/len ones in lens; its table replaces the code-length code's)
    return infl_build(W, W.lens, hlit, W.lit, INFL_LBITS, 0, 0, lane) &&
           infl_build(W, W.lens + hlit, hdist, W.dist, INFL_DBITS, 1, 1, lane);
}

__device__ bool infl_fixed(InflLds &W, uint32_t lane) {
    for (uint32_t s = lane; s < INFL_NLIT; s += 64) W.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
    if (lane < INFL_NDIST) W.lens[INFL_NLIT + lane] = 5;
    infl_sync();
    return infl_build(W, W.lens, INFL_NLIT, W.lit, INFL_LBITS, 0, 0, lane) &&
           infl_build(W, W.lens + INFL_NLIT, INFL_NDIST, W.dist, INFL_DBITS, 1, 1, lane);
}

// the first position after a NUL in src[p, n), n if there is none
__device__ uint64_t infl_skip_z(const uint8_t *src, uint64_t p, uint32_t n, uint32_t lane) {
    for (; p < n; p += 64) {
        const uint32_t c = p + lane < n ? src[p + lane] : 1u;
        const unsigned long long m = __ballot(c == 0);
        if (m) return p + (uint32_t)__builtin_ctzll(m) + 1;
    }
    return n;
}

// Inflate the member src[0, n) (infl_is_member holds) into dst[0, L): the view's length, or GM_NONE.
// Bounds: bits consumed <= 8 * (n - 8) (a token decoded past them is not emitted), bytes written
// <= L, every source of a copy inside [dst, dst + bytes written so far).
__device__ uint32_t infl_stream(InflLds &W, const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t L, uint32_t isize,
                                uint32_t lane) {
    const uint32_t flg = infl_u(src[3]);
    uint64_t pos = 10;
    if (flg & 4) pos += 2 + infl_u((uint32_t)src[10] | (uint32_t)src[11] << 8);   // FEXTRA
    if (flg & 8) pos = infl_skip_z(src, pos, n, lane);                              // FNAME
    if (flg & 16) pos = infl_skip_z(src, pos, n, lane);                             // FCOMMENT
    if (flg & 2) pos += 2;                                                          // FHCRC
    pos = uniform64(pos);
    if (pos > n - 8) return GM_NONE;
    const uint32_t skew = (uint32_t)((uintptr_t)src & 3);
    const uint8_t *base = src - skew;
    const uint64_t data_end = (uint64_t)skew + n - 8;   // the deflate data ends before CRC32 | ISIZE
    const uint64_t endbit = 8 * data_end;
    if (data_end > 0x7FFFFF00u) return GM_NONE;   // (32-bit buffer offsets: no view of a body that long)
    InflIn in;
    in.lane = lane;
    in.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(base), (short)0, (int)(skew + n), 0x00020000);
    infl_seek(in, skew + (uint32_t)pos);
    const bool room = L < isize;   // the limit cuts the stream: its first L bytes are the view
    uint32_t out = 0;
    bool last = false, cut = false;
    while (!last && !cut) {
        infl_refill(in);
        last = infl_bits(in, 1);
        const uint32_t type = infl_bits(in, 2);
        if (type == 3) return GM_NONE;
        if (type == 0) {   // stored: LEN | NLEN at the next byte, then LEN bytes, copied wave-wide
            infl_bits(in, in.bc & 7);
            infl_refill(in);
            const uint32_t len = infl_bits(in, 16), nlen = infl_bits(in, 16);
            if ((len ^ 0xFFFFu) != nlen) return GM_NONE;
            const uint64_t bp = infl_bitpos(in) >> 3;
            if (bp + len > data_end) return GM_NONE;
            uint32_t m = len;
            if (m > L - out) {
                if (!room) return GM_NONE;
                m = L - out;
                cut = true;
            }
            for (uint32_t j = lane; j < m; j += 64) dst[out + j] = base[bp + j];
            out += m;
            infl_seek(in, (uint32_t)bp + len);
            continue;
        }
        if (!(type == 1 ? infl_fixed(W, lane) : infl_dynamic(W, in, endbit, lane))) return GM_NONE;
        bool eob = false;
        while (!eob && !cut) {
            // ---- up to 64 tokens, decoded serially (uniform): token k into lane k of toks
            // literal: 1 | byte << 9 | 1 << 31;  match: length | distance << 9
            uint32_t toks = 0, ntok = 0, tot = 0;
            while (ntok < 64) {
                if (room && out + tot >= L) { cut = true; break; }
                infl_refill(in);
                uint32_t sym, tok = 0, tl = 0;
                if (!infl_sym(W, in, W.lit, INFL_LBITS, 0, sym)) return GM_NONE;
                if (sym < 256) {
                    tok = 1u | sym << 9 | 1u << 31;
                    tl = 1;
                } else if (sym == 256) {
                    eob = true;
                } else {
                    if (sym > 285) return GM_NONE;
                    const uint32_t s = sym - 257;
                    uint32_t len;
                    if (s < 8) len = s + 3;
                    else if (s == 28) len = 258;
                    else {
                        const uint32_t eb = (s - 4) >> 2;
                        len = ((4 + (s & 3)) << eb) + 3 + infl_bits(in, eb);
                    }
                    infl_refill(in);
                    uint32_t d;
                    if (!infl_sym(W, in, W.dist, INFL_DBITS, 1, d) || d > 29) return GM_NONE;
                    uint32_t dist = d + 1;
                    if (d >= 4) {
                        const uint32_t eb = (d >> 1) - 1;
                        dist = ((2 + (d & 1)) << eb) + 1 + infl_bits(in, eb);
                    }
                    if (dist > out + tot) return GM_NONE;   // before the start of the output
                    tok = len | dist << 9;
                    tl = len;
                }
                if (infl_bitpos(in) > endbit) return GM_NONE;   // out of input
                if (eob) break;
                if (tl > L - (out + tot)) {
                    if (!room) return GM_NONE;   // longer than ISIZE says
                    tl = L - (out + tot);
                    tok = (tok & ~511u) | tl;
                    cut = true;
                }
                toks = lane == ntok ? tok : toks;
                ntok++;
                tot += tl;
                if (cut) break;
            }
            // ---- resolved by all lanes
            const uint32_t tl = lane < ntok ? toks & 511 : 0u;
            const uint32_t at = out + infl_scan_incl(tl, lane) - tl;
            const bool lit = toks >> 31;
            if (lane < ntok && lit) dst[at] = (uint8_t)(toks >> 9);
            unsigned long long mm = __ballot(lane < ntok && !lit);
            if (mm) infl_drain();
            while (mm) {
                const int k = __builtin_ctzll(mm);
                mm &= mm - 1;
                const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)toks, k);
                const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)at, k);
                const uint32_t len = t & 511, dist = t >> 9;
                const uint8_t *s = dst + p - dist;
                if (dist >= len) {
                    for (uint32_t j = lane; j < len; j += 64) dst[p + j] = s[j];
                } else if (dist == 1) {
                    const uint8_t b = s[0];
                    for (uint32_t j = lane; j < len; j += 64) dst[p + j] = b;
                } else {
                    for (uint32_t j = lane; j < len; j += 64) dst[p + j] = s[j % dist];
                }
                infl_drain();   // this token's bytes before the next token reads them
            }
            out += tot;
        }
    }
    if (!cut && out != isize) return GM_NONE;
    return out;
}

__global__ void k_infl_reset(uint32_t *__restrict__ ctl) {
    if (threadIdx.x < INFL_CTL_WORDS) ctl[threadIdx.x] = 0;
}

// lim[i] = the slot of request i (0: not a gzip member, or -- with verdicts -- its location does
// not run the parser), len_out[i] = GM_NONE, the members' indices appended to list
__global__ void k_infl_size(const gm_req *__restrict__ reqs, const uint8_t *__restrict__ A, uint64_t alen,
                            const uint64_t *__restrict__ dlen, uint32_t n, const gm_verdict *__restrict__ verdicts,
                            const DLocUri *__restrict__ loc_uri, uint32_t n_locs, uint64_t *__restrict__ lim,
                            uint32_t *__restrict__ len_out, uint32_t *__restrict__ list, uint32_t *__restrict__ ctl) {
    const uint64_t len = dlen ? min(*dlen, alen) : alen;
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t i0 = blockIdx.x * blockDim.x; i0 < n; i0 += gridDim.x * blockDim.x) {
        const uint32_t i = i0 + threadIdx.x;
        bool gz = false;
        if (i < n) {
            bool run = true;
            if (verdicts) {
                const gm_verdict v = verdicts[i];
                run = waf_active(v) && v.location_id < n_locs &&
                      ((loc_uri[v.location_id].flags >> LOCURI_DEC_SHIFT) & DEC_GZIP);
            }
            uint64_t l = 0;
            if (run) {
                const Rec r = load_rec(reqs + i);
                const uint64_t body = r.base + r.uri_len + r.args_len + r.hdr_len;
                if (body + r.body_len <= len && infl_is_member(A + body, r.body_len)) {
                    gz = true;
                    l = infl_limit(infl_isize(A + body, r.body_len), r.body_len);
                }
            }
            lim[i] = l;
            len_out[i] = GM_NONE;
            if (i + 1 == n) lim[n] = 0;
        }
        const unsigned long long m = __ballot(gz);
        if (m) {
            uint32_t b = 0;
            if (lane == (uint32_t)__builtin_ctzll(m)) b = atomicAdd(ctl, (uint32_t)__popcll(m));
            b = __shfl(b, __builtin_ctzll(m));
            if (gz) list[b + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = i;
        }
    }
}

// persistent workgroups: each wave pulls the next listed body and inflates it into out[off[i] ...)
__global__ __launch_bounds__(INFL_BLOCK) void k_inflate(const gm_req *__restrict__ reqs, const uint8_t *__restrict__ A,
                                                         uint32_t n, const uint32_t *__restrict__ list,
                                                         uint32_t *__restrict__ ctl, uint8_t *__restrict__ out,
                                                         uint64_t out_cap, const uint64_t *__restrict__ off,
                                                         uint32_t *__restrict__ len_out, uint32_t *__restrict__ views,
                                                         uint32_t *__restrict__ ov) {
    __shared__ InflLds lds[INFL_WAVES];
    InflLds &W = lds[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t m = min(infl_u(ctl[0]), n);
    // The loop has one back edge and no lane-divergent branch at its level (every lane takes part in
    // the pop and in the result's store): a wave must stay whole from one stream to the next.
    for (;;) {
        const uint32_t q = infl_u(atomicAdd(ctl + 1, lane == 0 ? 1u : 0u));   // (lane 0: the value before the wave's add)
        if (q >= m) break;
        const uint32_t i = min(infl_u(list[q]), n - 1);
        const Rec r = load_rec(reqs + i);
        const uint32_t blen = infl_u(r.body_len);
        const uint8_t *src = A + uniform64(r.base + r.uri_len + r.args_len + r.hdr_len);
        const uint32_t isize = infl_u(infl_isize(src, blen));
        const uint32_t L = infl_limit(isize, blen);
        const uint64_t o = uniform64(off[i]);
        const bool fits = o + L <= out_cap;
        uint32_t res = GM_NONE;
        if (fits) res = infl_u(infl_stream(W, src, blen, out + o, L, isize, lane));
        len_out[i] = res;   // (the same word from every lane: one store)
        atomicAdd(views, lane == 0 && res != GM_NONE ? 1u : 0u);
        atomicOr(ov, lane == 0 && !fits ? 1u : 0u);
    }
}
