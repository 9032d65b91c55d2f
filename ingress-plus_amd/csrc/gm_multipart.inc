// gm_multipart.inc -- the multipart request parser (SURVEY.md §8 f4, Wallarm's `multipart` parser),
// included into gm_device.hip's anonymous namespace: the part views of a multipart/form-data body,
// one wave (64 lanes) per body.
//
// THE GRAMMAR (include/gpumatch.h states the same; tests/test_gpu_multipart.py restates it in Python)
// Which bodies.  The request's first Content-Type header (the one body_kind reads), its value
//   trimmed as nginx trims it.  The value starts with "multipart/" (ASCII case-insensitive).  After
//   its first ';', the first case-insensitive "boundary=" that is preceded by ';', space or tab.  If
//   the next byte is '"' the boundary B is the bytes up to the next '"' (or the value's end);
//   otherwise the bytes up to the first ';', space, tab or the value's end.  1 <= |B| <= 70, else
//   the body is not multipart.  The body is read as sent (a gzip body is not inflated first).
// Delimiter.  D = "--" B counts only at body offset 0 or directly after '\n', and only if followed by
//   "--" (the close delimiter: everything after it is ignored) or by any run of space, tab, '\r' and
//   then '\n' (a part begins after that '\n').  Any other continuation: the bytes are content.
//   Bytes before the first delimiter are ignored; a body with no delimiter has no view (GM_NONE);
//   without a close delimiter the last part runs to the body's end.
// A part is the bytes from its start to the next delimiter's D, minus one trailing '\n' if there is
//   one and then one trailing '\r' if there is one.  Its lines end at '\n' (a '\r' before it is not
//   part of the line).  The header block ends at the first empty line that has its '\n' inside the
//   part; the content follows it.  A part with no empty line has headers only and no content.  No
//   folding.  Of each recognised header the part's first line counts, matched at the line's start
//   by case-insensitive name and ':':
//   Content-Disposition: its value is read left to right for parameters: "name=", "filename=" or
//     "filename*=" (case-insensitive) preceded by ';', space or tab.  The value of name / filename
//     is a quoted string if it starts with '"' (it ends at the next '"' not preceded by a pairing
//     '\', or at the line's end; \x becomes x, a '\' that is the line's last byte stays), else a
//     token that ends at ';', space, tab, '\r' or the line's end.  The value of filename*= is always
//     a token; the bytes after its second ''' are percent-decoded (%XY, two hex digits); with fewer
//     than two ''' it yields nothing.  The read resumes after the value, so a parameter name inside
//     another parameter's value is not a parameter.  The first of each kind is taken.
//   Content-Type: the part is JSON if the value contains "json", case-insensitively.
//   Content-Transfer-Encoding: the value without leading / trailing spaces and tabs equals "base64"
//     or "quoted-printable", case-insensitively.
//   The first GM_MULTIPART_PARTS (64) parts are taken; later ones are ignored.
// The view M.  For each taken part in order, each of these that is present, followed by '\n': name,
//   filename, the decoded filename*, the content (present if the part has an empty line) under its
//   transfer encoding:
//   base64: every byte outside [A-Za-z0-9+/] is skipped, each full 4-character quantum of the rest
//     is decoded, a partial quantum at the end is ignored;
//   quoted-printable: "=XY" (two hex digits) is the byte, '=' before "\r\n" or "\n" is removed with
//     the line end, every other byte (a lone '=' too) stays;
//   otherwise verbatim.
// flags = taken parts << 8 | (any taken part is JSON).
//
// SIZE BOUND: |M| <= body_len, so request i's slot is body_len bytes.  Every taken part follows a
// delimiter line "--" B ... '\n' of >= 4 bytes that belongs to no part; it pays for the '\n' after the
// content, and no decoding lengthens content (base64 4 -> 3, "=XY" 3 -> 1, verbatim 1 -> 1).  The
// parameters of one Content-Disposition line are read left to right and never overlap, so each
// emitted value comes from body bytes of its own; a value never grows (\x -> x, %XY -> byte) and the
// '\n' after it is paid by the >= 5 bytes of "name=" / "filename=" / "filename*=", which are not
// emitted.  Header bytes and content bytes of a part are disjoint, parts are disjoint.
//
// WORK SPLIT.  k_mp_size (a lane per request) parses the boundary and lists the multipart bodies;
// k_multipart's persistent workgroups pull from the list, a wave owning a body.  (1) Delimiter
// search, 1 KiB a step: lane l loads 16 bytes through a buffer resource over the body's 16-byte
// granules (a read past it returns 0), turns them into a '\n' and a '-' bit mask, takes the two bits
// it needs from lane l - 1 (the step's last lane carries into the next step) and marks where "\n--"
// ends; the marks are walked wave-uniformly and each candidate is verified by all lanes (lane k
// holds D[k] and D[64 + k] in registers; one ballot a round).  Parts go into a 64-entry table in LDS.
// (2) Per part the header lines are found by ballot, the three names matched by a lane-parallel
// compare, parameters by ballot on '='.  (3) Emission: wave-wide verbatim copy (16 bytes a lane once
// the destination is aligned, source dwords funnel-shifted), base64 by ballot / mbcnt compaction into
// an LDS row and a quantum a lane, quoted-printable and percent by per-byte lookahead and a ballot
// rank.  Every write to memory is a vector store.

#ifndef GM_MULTIPART_PARTS
#define GM_MULTIPART_PARTS 64
#endif
constexpr uint32_t MP_BLOCK = 256, MP_WAVES = MP_BLOCK / 64;
constexpr uint32_t MP_BMAX = 70;
// control words of one launch: [0] bodies listed, [1] the list's queue head, [2] views given, [3] overflow
constexpr uint32_t MP_CTL_WORDS = 4;
constexpr uint32_t MP_VIEWS_WORD = 25;                      // batch status word: bodies given a view
constexpr uint32_t MP_STATUS_WORD = UPURI_STATUS_WORD + 2;  // gm_multipart_bodies: output capacity exceeded

struct MpLds {                                  // one wave's
    uint2 tab[GM_MULTIPART_PARTS];              // parts: {start, end} in the body
    uint8_t stage[72];                          // base64: the alphabet values of a chunk, compacted
};
static_assert(sizeof(MpLds) * MP_WAVES <= 20 * 1024, "at least the inflate kernel's 8 workgroups per CU");

struct MpIn {
    __amdgpu_buffer_rsrc_t rs;   // the body's 16-byte granules
    uint32_t skew, n, lane;      // the body is bytes [skew, skew + n) of the resource
};
__device__ __forceinline__ uint32_t mp_rank(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// body byte p (0 past the end), per lane / the same p in every lane
__device__ __forceinline__ uint32_t mp_b(const MpIn &in, uint32_t p) {
    return p < in.n ? (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(in.rs, (int)(in.skew + p), 0, 0) : 0u;
}
__device__ __forceinline__ uint32_t mp_bu(const MpIn &in, uint32_t p) { return infl_u(mp_b(in, p)); }
__device__ __forceinline__ bool mp_ws(uint32_t c) { return c == ' ' || c == '\t'; }
__device__ __forceinline__ bool mp_sep(uint32_t c) { return c == ';' || c == ' ' || c == '\t'; }

// the first position in [from, to) whose byte satisfies pred, `to` if none (to <= n)
template <class F>
__device__ __forceinline__ uint32_t mp_find(const MpIn &in, uint32_t from, uint32_t to, F pred) {
    for (uint32_t p = from; p < to; p += 64) {
        const uint32_t q = p + in.lane;
        const uint32_t c = mp_b(in, q);
        const unsigned long long m = __ballot(q < to && pred(c));
        if (m) return p + (uint32_t)__builtin_ctzll(m);
    }
    return to;
}

__device__ __forceinline__ void mp_put(uint8_t *dst, uint32_t &o, uint32_t c, uint32_t lane) {
    if (lane == 0) dst[o] = (uint8_t)c;
    o++;
}

// body[a, e) -> dst + o verbatim
__device__ void mp_copy(const MpIn &in, uint32_t a, uint32_t e, uint8_t *dst, uint32_t &o) {
    uint32_t len = e - a;
    uint8_t *d = dst + o;
    o += len;
    const uint32_t head = min(len, (uint32_t)(-(uintptr_t)d & 15));
    if (in.lane < head) d[in.lane] = (uint8_t)mp_b(in, a + in.lane);
    a += head; d += head; len -= head;
    const uint32_t r = in.skew + a, sh = (r & 3) * 8, nv = len / 16;
    for (uint32_t v = in.lane; v < nv; v += 64) {
        const uint32_t off = (r & ~3u) + v * 16;
        uint32_t w[5];
#pragma unroll
        for (uint32_t j = 0; j < 5; j++) w[j] = __builtin_amdgcn_raw_buffer_load_b32(in.rs, (int)(off + 4 * j), 0, 0);
        if (sh) {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) w[j] = w[j] >> sh | w[j + 1] << (32 - sh);
        }
        *reinterpret_cast<uint4 *>(d + (size_t)v * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    const uint32_t done = nv * 16;
    if (in.lane < len - done) d[done + in.lane] = (uint8_t)mp_b(in, a + done + in.lane);
}

// the escape that starts with byte c0 == E, followed by c1 c2: its length (0: none)
__device__ __forceinline__ uint32_t mp_esc_len(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t E, bool qp) {
    if (c0 != E) return 0;
    if (dec_hexv(c1) >= 0 && dec_hexv(c2) >= 0) return 3;
    if (qp && c1 == '\r' && c2 == '\n') return 3;
    if (qp && c1 == '\n') return 2;
    return 0;
}
// body[a, e) -> dst + o, quoted-printable (qp) or percent decoded.  The bytes an escape consumes are
// hex digits, '\r' or '\n', never the escape character: every lane decides from its own lookahead.
__device__ void mp_esc(const MpIn &in, uint32_t a, uint32_t e, uint8_t *dst, uint32_t &o, bool qp) {
    const uint32_t E = qp ? '=' : '%';
    for (uint32_t p0 = a; p0 < e; p0 += 64) {
        const uint32_t p = p0 + in.lane;
        uint32_t c[5];   // bytes p - 2 .. p + 2, 0 outside [a, e)
#pragma unroll
        for (uint32_t j = 0; j < 5; j++) {
            const uint32_t q = p + j - 2;
            c[j] = (p + j >= a + 2 && q < e) ? mp_b(in, q) : 0u;
        }
        const uint32_t l0 = mp_esc_len(c[2], c[3], c[4], E, qp), l1 = mp_esc_len(c[1], c[2], c[3], E, qp),
                       l2 = mp_esc_len(c[0], c[1], c[2], E, qp);
        const bool consumed = l1 >= 2 || l2 == 3;
        const int h = dec_hexv(c[3]), l = dec_hexv(c[4]);
        const bool byte_esc = l0 && h >= 0 && l >= 0;
        const bool keep = p < e && !consumed && (l0 == 0 || byte_esc);
        const unsigned long long m = __ballot(keep);
        if (keep) dst[o + mp_rank(m)] = (uint8_t)(byte_esc ? (uint32_t)(h << 4 | l) : c[2]);
        o += (uint32_t)__popcll(m);
    }
}

// body[a, e) -> dst + o, base64: the alphabet bytes compacted into the LDS row, a quantum a lane
__device__ void mp_b64(const MpIn &in, MpLds &W, uint32_t a, uint32_t e, uint8_t *dst, uint32_t &o) {
    uint32_t cnt = 0;   // the partial quantum carried from the chunk before (in stage[0, cnt))
    for (uint32_t p0 = a; p0 < e; p0 += 64) {
        const uint32_t p = p0 + in.lane;
        const int v = p < e ? b64v(mp_b(in, p)) : -1;
        const unsigned long long m = __ballot(v >= 0);
        if (v >= 0) W.stage[cnt + mp_rank(m)] = (uint8_t)v;
        const uint32_t total = cnt + (uint32_t)__popcll(m), nq = total >> 2, rem = total & 3;
        infl_sync();
        if (in.lane < nq) {
            const uint8_t *s = W.stage + 4 * in.lane;
            const uint32_t x = (uint32_t)s[0] << 18 | (uint32_t)s[1] << 12 | (uint32_t)s[2] << 6 | (uint32_t)s[3];
            uint8_t *d = dst + o + 3 * in.lane;
            d[0] = (uint8_t)(x >> 16); d[1] = (uint8_t)(x >> 8); d[2] = (uint8_t)x;
        }
        const uint32_t t = in.lane < rem ? W.stage[4 * nq + in.lane] : 0u;
        infl_sync();
        if (in.lane < rem) W.stage[in.lane] = (uint8_t)t;
        infl_sync();
        o += 3 * nq;
        cnt = rem;
    }
}

// a quoted string's bytes from s (after the opening '"') within the line [.., le): returns the position
// after the closing '"' (or le); with dst, the unescaped bytes -> dst + o.  The one lane-serial loop
// over header bytes: a value's bytes come 64 at a time into a register and are read by readlane,
// the output collects in a register and leaves 64 bytes a store.
__device__ uint32_t mp_quoted(const MpIn &in, uint32_t s, uint32_t le, uint8_t *dst, uint32_t &o) {
    uint32_t i = s, chunk = 0, outv = 0, k = 0;
    bool esc = false;
    while (i < le) {
        const uint32_t at = (i - s) & 63;
        if (at == 0) chunk = i + in.lane < le ? mp_b(in, i + in.lane) : 0u;
        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)chunk, (int)infl_u(at));
        i++;
        if (!esc) {
            if (c == '"') break;
            if (c == '\\' && i < le) { esc = true; continue; }
        }
        esc = false;
        outv = in.lane == k ? c : outv;
        k++;
        if (k == 64) {
            if (dst) dst[o + in.lane] = (uint8_t)outv;
            o += 64;
            k = 0;
        }
    }
    if (dst && in.lane < k) dst[o + in.lane] = (uint8_t)outv;
    o += k;
    return i;
}

__device__ const uint8_t MP_HDR[3][32] = {"content-disposition:", "content-type:", "content-transfer-encoding:"};
__device__ const uint8_t MP_PAR[2][16] = {"?filename*", "??filename"};
__device__ const uint8_t MP_ENC[2][20] = {"base64", "quoted-printable"};

// The part body[ps, pe): its headers read, its pieces of the view -> dst + o; json |= a JSON part.
__device__ void mp_part(const MpIn &in, MpLds &W, uint32_t ps, uint32_t pe, uint8_t *dst, uint32_t &o, bool &json) {
    const uint32_t lane = in.lane;
    uint32_t v_name = GM_NONE, e_name = 0, v_file = GM_NONE, e_file = 0, v_ext = GM_NONE, e_ext = 0;
    bool q_name = false, q_file = false, seen_cd = false, seen_ct = false, seen_cte = false;
    uint32_t enc = 0, cs = GM_NONE;
    uint32_t q = ps;
    while (q < pe) {
        const uint32_t e = mp_find(in, q, pe, [](uint32_t c) { return c == '\n'; });
        uint32_t le = e;
        if (le > q && mp_bu(in, le - 1) == '\r') le--;
        if (e < pe && le == q) { cs = e + 1; break; }   // the empty line
        // the header's name: lane k against byte k of the three names
        const uint32_t hc = q + lane < le ? lc(mp_b(in, q + lane)) : 0u;
        const uint32_t l32 = lane & 31;
        const bool is_cd = (uint32_t)__ballot(lane < 20 && hc == MP_HDR[0][l32]) == 0xFFFFFu;
        const bool is_ct = (uint32_t)__ballot(lane < 13 && hc == MP_HDR[1][l32]) == 0x1FFFu;
        const bool is_cte = (uint32_t)__ballot(lane < 26 && hc == MP_HDR[2][l32]) == 0x3FFFFFFu;
        if (is_cd && !seen_cd) {
            seen_cd = true;
            uint32_t skip = q + 20;   // the read resumes here: '=' before it lie in a value
            for (uint32_t p0 = q + 20; p0 < le; p0 += 64) {
                unsigned long long m = __ballot(p0 + lane < le && mp_b(in, p0 + lane) == '=');
                while (m) {
                    const uint32_t x = p0 + (uint32_t)__builtin_ctzll(m);
                    m &= m - 1;
                    if (x < skip) continue;
                    // lanes 0..9: the ten bytes before the '=' ("?filename*" / "??filename", ? a separator)
                    const uint32_t w = lane < 10 ? lc(mp_b(in, x - 10 + lane)) : 0u;
                    const uint32_t l16 = lane & 15;
                    const uint32_t ma = (uint32_t)__ballot(lane < 10 && (lane == 0 ? mp_sep(w) : w == MP_PAR[0][l16]));
                    const uint32_t mb = (uint32_t)__ballot(lane < 10 && (lane == 1 ? mp_sep(w) : w == MP_PAR[1][l16]));
                    const uint32_t mc = (uint32_t)__ballot(lane < 10 && (lane == 5 ? mp_sep(w) : w == MP_PAR[1][l16]));
                    const bool is_ext = (ma & 0x3FFu) == 0x3FFu, is_file = (mb & 0x3FEu) == 0x3FEu,
                               is_name = (mc & 0x3E0u) == 0x3E0u;
                    if (!is_ext && !is_file && !is_name) continue;
                    uint32_t v0 = x + 1, ve;
                    const bool quoted = !is_ext && v0 < le && mp_bu(in, v0) == '"';
                    if (quoted) {
                        uint32_t none = 0;
                        v0++;
                        ve = mp_quoted(in, v0, le, nullptr, none);
                    } else {
                        ve = mp_find(in, v0, le, [](uint32_t c) { return mp_sep(c) || c == '\r' || c == '\n'; });
                    }
                    skip = ve;
                    if (is_name && v_name == GM_NONE) { v_name = v0; e_name = ve; q_name = quoted; }
                    if (is_file && v_file == GM_NONE) { v_file = v0; e_file = ve; q_file = quoted; }
                    if (is_ext && v_ext == GM_NONE) { v_ext = v0; e_ext = ve; }
                }
            }
        } else if (is_ct && !seen_ct) {
            seen_ct = true;
            for (uint32_t p0 = q + 13; p0 < le; p0 += 64) {
                const uint32_t p = p0 + lane;
                const bool hit = p + 4 <= le && lc(mp_b(in, p)) == 'j' && lc(mp_b(in, p + 1)) == 's' &&
                                 lc(mp_b(in, p + 2)) == 'o' && lc(mp_b(in, p + 3)) == 'n';
                if (__ballot(hit)) { json = true; break; }
            }
        } else if (is_cte && !seen_cte) {
            seen_cte = true;
            const uint32_t a = mp_find(in, q + 26, le, [](uint32_t c) { return !mp_ws(c); });
            const uint32_t w = a + lane < le ? lc(mp_b(in, a + lane)) : 0u;
            const uint32_t l20 = lane < 20 ? lane : 0u;
            const bool b64 = (uint32_t)__ballot(lane < 6 && w == MP_ENC[0][l20]) == 0x3Fu;
            const bool qpr = (uint32_t)__ballot(lane < 16 && w == MP_ENC[1][l20]) == 0xFFFFu;
            const uint32_t wl = b64 ? 6u : 16u;
            if ((b64 || qpr) && mp_find(in, a + wl, le, [](uint32_t c) { return !mp_ws(c); }) == le) enc = b64 ? 1u : 2u;
        }
        q = e + 1;
    }
    // ---- the part's pieces, each followed by '\n'
    if (v_name != GM_NONE) {
        if (q_name) mp_quoted(in, v_name, e_name, dst, o); else mp_copy(in, v_name, e_name, dst, o);
        mp_put(dst, o, '\n', lane);
    }
    if (v_file != GM_NONE) {
        if (q_file) mp_quoted(in, v_file, e_file, dst, o); else mp_copy(in, v_file, e_file, dst, o);
        mp_put(dst, o, '\n', lane);
    }
    if (v_ext != GM_NONE) {
        const uint32_t t0 = mp_find(in, v_ext, e_ext, [](uint32_t c) { return c == '\''; });
        const uint32_t t1 = t0 < e_ext ? mp_find(in, t0 + 1, e_ext, [](uint32_t c) { return c == '\''; }) : e_ext;
        if (t1 < e_ext) {
            mp_esc(in, t1 + 1, e_ext, dst, o, false);
            mp_put(dst, o, '\n', lane);
        }
    }
    if (cs != GM_NONE) {
        if (enc == 1) mp_b64(in, W, cs, pe, dst, o);
        else if (enc == 2) mp_esc(in, cs, pe, dst, o, true);
        else mp_copy(in, cs, pe, dst, o);
        mp_put(dst, o, '\n', lane);
    }
}

struct MpScan {
    uint32_t np, start;   // parts begun; the open part's start
    bool open, done, found;
};
// the part's end: p without one trailing '\n', then without one trailing '\r'
__device__ __forceinline__ uint32_t mp_trim(const MpIn &in, uint32_t start, uint32_t p) {
    if (p > start && mp_bu(in, p - 1) == '\n') p--;
    if (p > start && mp_bu(in, p - 1) == '\r') p--;
    return p;
}
// a candidate: "--" at p, at offset 0 or after '\n'.  All lanes compare D (d0: bytes 0..63, d1: 64..71).
__device__ void mp_cand(const MpIn &in, MpLds &W, MpScan &S, uint32_t p, uint32_t d0, uint32_t d1, uint32_t dl) {
    const uint32_t lane = in.lane;
    if (S.done || p + dl > in.n) return;
    if (__ballot(lane < dl && mp_b(in, p + lane) != d0)) return;
    if (dl > 64 && __ballot(64 + lane < dl && mp_b(in, p + 64 + lane) != d1)) return;
    const uint32_t t = p + dl;
    const bool close = mp_bu(in, t) == '-' && mp_bu(in, t + 1) == '-';
    uint32_t u = t;
    if (!close) {
        u = mp_find(in, t, in.n, [](uint32_t c) { return !(mp_ws(c) || c == '\r'); });
        if (u >= in.n || mp_bu(in, u) != '\n') return;   // not a delimiter: content
    }
    S.found = true;
    if (S.open) {
        if (lane == 0) W.tab[S.np - 1] = make_uint2(S.start, mp_trim(in, S.start, p));
        S.open = false;
    }
    if (close || S.np == GM_MULTIPART_PARTS) { S.done = true; return; }
    S.start = u + 1;
    S.open = true;
    S.np++;
}

// The view of the body src[0, n) with boundary bnd[0, bl) -> dst[0, <= n): its length, or GM_NONE.
__device__ uint32_t mp_body(MpLds &W, const uint8_t *src, uint32_t n, const uint8_t *bnd, uint32_t bl, uint8_t *dst,
                            uint32_t lane, uint32_t &flags) {
    MpIn in;
    in.lane = lane;
    in.skew = (uint32_t)((uintptr_t)src & 15);
    in.n = n;
    const uint64_t total64 = (uint64_t)in.skew + n;
    if (n == 0 || total64 > 0x7FFFFF00u) return GM_NONE;   // (32-bit buffer offsets: no view of a body that long)
    const uint32_t total = (uint32_t)total64;
    in.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(src - in.skew), (short)0, (int)((total + 15) & ~15u), 0x00020000);
    const uint32_t dl = bl + 2;
    const uint32_t d0 = lane < 2 ? (uint32_t)'-' : (lane < dl ? (uint32_t)bnd[lane - 2] : 0u);
    const uint32_t d1 = 64 + lane < dl ? (uint32_t)bnd[62 + lane] : 0u;
    MpScan S{0, 0, false, false, false};
    mp_cand(in, W, S, 0, d0, d1, dl);
    // ---- the search: marks where "\n--" ends, resource byte r = r0 + 16 * lane + j <-> bit j
    uint32_t carry_n = 0, carry_d = 0;
    for (uint32_t r0 = 0; r0 < total && !S.done; r0 += 1024) {
        const uint32_t off = r0 + 16 * lane;
        uint32_t w[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) w[j] = __builtin_amdgcn_raw_buffer_load_b32(in.rs, (int)(off + 4 * j), 0, 0);
        uint32_t mn = 0, md = 0;
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) {
            const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 0xFF;
            mn |= (c == '\n' ? 1u : 0u) << j;
            md |= (c == '-' ? 1u : 0u) << j;
        }
        uint32_t pn = __shfl_up(mn, 1), pd = __shfl_up(md, 1);   // the lane before: its last two bytes matter
        if (lane == 0) { pn = carry_n; pd = carry_d; }
        carry_n = (uint32_t)__builtin_amdgcn_readlane((int)mn, 63);
        carry_d = (uint32_t)__builtin_amdgcn_readlane((int)md, 63);
        const uint32_t en = mn << 2 | pn >> 14, ed = md << 2 | pd >> 14;   // bit i <-> byte off - 2 + i
        uint32_t marks = en & (ed >> 1) & (ed >> 2) & 0xFFFFu;
        // inside the body: the '\n' at r - 2 >= skew, the second '-' at r < total
        const uint32_t lo = in.skew + 2 > off ? min(in.skew + 2 - off, 16u) : 0u;
        const uint32_t hi = total > off ? min(total - off, 16u) : 0u;
        marks &= ((1u << hi) - 1) & ~((1u << lo) - 1);
        unsigned long long any = __ballot(marks != 0);
        while (any && !S.done) {
            const uint32_t L = (uint32_t)__builtin_ctzll(any);
            any &= any - 1;
            uint32_t mm = (uint32_t)__builtin_amdgcn_readlane((int)marks, (int)L);
            while (mm && !S.done) {
                const uint32_t j = (uint32_t)__builtin_ctz(mm);
                mm &= mm - 1;
                mp_cand(in, W, S, r0 + 16 * L + j - 1 - in.skew, d0, d1, dl);
            }
        }
    }
    if (!S.found) return GM_NONE;
    if (S.open && lane == 0) W.tab[S.np - 1] = make_uint2(S.start, mp_trim(in, S.start, n));
    infl_sync();
    uint32_t o = 0;
    bool json = false;
    for (uint32_t k = 0; k < S.np; k++) {
        const uint2 pt = W.tab[k];
        mp_part(in, W, infl_u(pt.x), infl_u(pt.y), dst, o, json);
    }
    flags = S.np << 8 | (json ? 1u : 0u);
    return o;
}

// the boundary of a multipart body from the first Content-Type line: its arena offset and length
// (0: not a multipart body)
__device__ uint32_t mp_boundary(const uint8_t *A, const Rec &r, uint64_t hdrs, uint64_t &at) {
    HdrIt it{hdrs, hdrs + r.hdr_len};
    uint64_t ns, vs; uint32_t nl, vl;
    const uint8_t ct[13] = "content_type";
    while (hdr_next(A, it, ns, nl, vs, vl)) {
        if (!hdr_name_is(A, ns, nl, ct, 12)) continue;
        const char *mp = "multipart/", *bd = "boundary=";
        if (vl < 10) return 0;
        for (uint32_t k = 0; k < 10; k++) if (lc(A[vs + k]) != (uint32_t)(uint8_t)mp[k]) return 0;
        uint32_t s = 10;
        while (s < vl && A[vs + s] != ';') s++;
        for (uint32_t k = s + 1; k + 9 <= vl; k++) {
            if (!mp_sep(A[vs + k - 1])) continue;
            bool ok = true;
            for (uint32_t j = 0; ok && j < 9; j++) ok = lc(A[vs + k + j]) == (uint32_t)(uint8_t)bd[j];
            if (!ok) continue;
            uint32_t b = k + 9, e;
            if (b < vl && A[vs + b] == '"') {
                b++;
                for (e = b; e < vl && A[vs + e] != '"'; e++) {}
            } else {
                for (e = b; e < vl && !mp_sep(A[vs + e]); e++) {}
            }
            at = vs + b;
            return e - b <= MP_BMAX ? e - b : 0u;
        }
        return 0;
    }
    return 0;
}

__global__ void k_mp_reset(uint32_t *__restrict__ ctl) {
    if (threadIdx.x < MP_CTL_WORDS) ctl[threadIdx.x] = 0;
}

// lim[i] = the slot of request i (its body_len; 0: not multipart, or -- with verdicts -- its location
// does not run the parser), bnd[i] = the boundary's arena offset | its length << 56, len_out[i] =
// GM_NONE, flags_out[i] = 0, the multipart bodies' indices appended to list
__global__ void k_mp_size(const gm_req *__restrict__ reqs, const uint8_t *__restrict__ A, uint64_t alen,
                          const uint64_t *__restrict__ dlen, uint32_t n, const gm_verdict *__restrict__ verdicts,
                          const DLocUri *__restrict__ loc_uri, uint32_t n_locs, uint64_t *__restrict__ lim,
                          uint64_t *__restrict__ bnd, uint32_t *__restrict__ len_out, uint32_t *__restrict__ flags_out,
                          uint32_t *__restrict__ list, uint32_t *__restrict__ ctl) {
    const uint64_t len = dlen ? min(*dlen, alen) : alen;
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t i0 = blockIdx.x * blockDim.x; i0 < n; i0 += gridDim.x * blockDim.x) {
        const uint32_t i = i0 + threadIdx.x;
        bool mp = false;
        if (i < n) {
            bool run = true;
            if (verdicts) {
                const gm_verdict v = verdicts[i];
                run = waf_active(v) && v.location_id < n_locs &&
                      ((loc_uri[v.location_id].flags >> LOCURI_DEC_SHIFT) & DEC_MULTIPART);
            }
            uint64_t l = 0, at = 0;
            if (run) {
                const Rec r = load_rec(reqs + i);
                const uint64_t hdrs = r.base + r.uri_len + r.args_len, body = hdrs + r.hdr_len;
                if (r.body_len && body + r.body_len <= len) {
                    const uint32_t bl = mp_boundary(A, r, hdrs, at);
                    if (bl) {
                        mp = true;
                        l = r.body_len;
                        at |= (uint64_t)bl << 56;
                    }
                }
            }
            lim[i] = l;
            bnd[i] = at;
            len_out[i] = GM_NONE;
            flags_out[i] = 0;
            if (i + 1 == n) lim[n] = 0;
        }
        const unsigned long long m = __ballot(mp);
        if (m) {
            uint32_t b = 0;
            if (lane == (uint32_t)__builtin_ctzll(m)) b = atomicAdd(ctl, (uint32_t)__popcll(m));
            b = __shfl(b, __builtin_ctzll(m));
            if (mp) list[b + mp_rank(m)] = i;
        }
    }
}

// persistent workgroups: each wave pulls the next listed body and writes its view to out[off[i] ...)
__global__ __launch_bounds__(MP_BLOCK) void k_multipart(const gm_req *__restrict__ reqs, const uint8_t *__restrict__ A,
                                                         uint32_t n, const uint32_t *__restrict__ list,
                                                         uint32_t *__restrict__ ctl, const uint64_t *__restrict__ bnd,
                                                         uint8_t *__restrict__ out, uint64_t out_cap,
                                                         const uint64_t *__restrict__ off, uint32_t *__restrict__ len_out,
                                                         uint32_t *__restrict__ flags_out, uint32_t *__restrict__ views,
                                                         uint32_t *__restrict__ ov) {
    __shared__ MpLds lds[MP_WAVES];
    MpLds &W = lds[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t m = min(infl_u(ctl[0]), n);
    // As in k_inflate: one back edge, no lane-divergent branch at the loop's level (every lane takes
    // part in the pop, the result's stores and the counters), so a wave stays whole between bodies.
    for (;;) {
        const uint32_t q = infl_u(atomicAdd(ctl + 1, lane == 0 ? 1u : 0u));   // (lane 0: the value before the wave's add)
        if (q >= m) break;
        const uint32_t i = min(infl_u(list[q]), n - 1);
        const Rec r = load_rec(reqs + i);
        const uint32_t blen = infl_u(r.body_len);
        const uint8_t *src = A + uniform64(r.base + r.uri_len + r.args_len + r.hdr_len);
        const uint64_t b = uniform64(bnd[i]);
        const uint32_t bl = min((uint32_t)(b >> 56), MP_BMAX);
        const uint64_t o = uniform64(off[i]);
        const bool fits = o + blen <= out_cap;
        uint32_t res = GM_NONE, flags = 0;
        if (fits) res = infl_u(mp_body(W, src, blen, A + (b & 0x00FFFFFFFFFFFFFFull), bl, out + o, lane, flags));
        flags = infl_u(flags);
        len_out[i] = res;   // (the same word from every lane: one store)
        flags_out[i] = res != GM_NONE ? flags : 0u;
        atomicAdd(views, lane == 0 && res != GM_NONE ? 1u : 0u);
        atomicOr(ov, lane == 0 && !fits ? 1u : 0u);
    }
}
