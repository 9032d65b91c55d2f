// gm_wire.inc -- HTTP/1.x wire parser (SURVEY.md §8 f2), included into gm_device.hip's anonymous
// namespace.  Raw request bytes -> gm_req records + the packed payload arena gm_match_batch reads.
//
// nginx 1.17.3's intake, restated (the semantics and their divergences are listed at
// orc_parse_one in oracle/gm_oracle.c, the C restatement the tests check this against):
// ngx_http_parse_request_line, ngx_http_parse_complex_uri ($uri, the same un_one as
// gm_normalize_uris), ngx_http_parse_header_line + ngx_http_process_request_headers
// (ignore_invalid_headers on, underscores_in_headers off), Host / Content-Length /
// Transfer-Encoding rules, the chunked body decoder.
//
// Layout: a WAVE per request.  (1) The wave streams the message in 1 KiB windows (16 B a lane),
// finds every LF with a per-lane mask, compacts their positions in order into an LDS line table
// (mbcnt-style wave prefix) and stops at the empty line that ends the header.  (2) Lane 0 parses
// the request line; meanwhile lane j parses header lines j+1, j+65, ... (name check, ':' and
// value bounds, Host / Content-Length / Transfer-Encoding), and wave reductions combine their
// verdicts.  (3) The body: Content-Length bytes, or chunks walked by lane 0 and copied by the wave.
// Two launches: pass 1 only sizes each record (bound: the path's raw length stands for $uri);
// an exclusive scan turns sizes into 16-B aligned bases; pass 2 re-parses and writes the fields
// (header lines at wave-prefix offsets), zero-fills the slack of its slot and the gm_req.
// Bound: HBM for the copies; the per-line work is a lane per line, the request line a lane.

constexpr int WIRE_WAVES = 4;                 // waves per 256-thread block
constexpr uint32_t WIRE_LINES = 256;          // line table per wave: request line + 254 headers + end
constexpr uint32_t WIRE_SCR = 8192 + 64;      // per-wave $uri scratch (global memory) bytes
// the parse is latency-bound (dependent global / LDS loads, lane-serial phases): occupancy
// against registers -- 6 waves per SIMD (<= 80 VGPRs: pass 1 stops spilling most of its 74)
// parse 2M messages in 20.2 ms per call against 22.1 at 8 and 22.8 at 4 (r6h, one box)
#ifndef GM_WIRE_WPE
#define GM_WIRE_WPE 6
#endif
#ifndef GM_WIRE_WPE_EMIT
#define GM_WIRE_WPE_EMIT GM_WIRE_WPE
#endif
#ifndef GM_WIRE_CANON
#define GM_WIRE_CANON 1                       // (0: always the per-line header emit; measurement)
#endif
#define WIRE_OCC __attribute__((amdgpu_waves_per_eu(GM_WIRE_WPE)))
#define WIRE_OCC_EMIT __attribute__((amdgpu_waves_per_eu(GM_WIRE_WPE_EMIT)))
constexpr uint32_t WIRE_STAGE = 2048;         // message bytes staged in LDS per wave (the header)
constexpr uint32_t WIRE_PIECES = 8;           // a chunked body's chunks pass 1 records for pass 2
// k_wire_proxy's descriptor flags (below): paddr fields valid; a broken PROXY header (444)
constexpr uint8_t WIRE_F_PADDR = 0x20, WIRE_F_BROKEN = 0x80;
constexpr uint32_t PADDR_MAX = 46;

struct WireOut {                              // what a pass knows about one request
    uint32_t status;                          // 0 ok, else the HTTP status (GM_REQ_INVALID)
    uint32_t minor;
    uint32_t method_off, method_len;          // offsets relative to the message start
    uint32_t target_off, target_len;          // $request_uri ("/" if absolute-form has no path)
    uint32_t path_off, path_len;
    uint32_t args_off, args_len;
    uint32_t host_off, host_len;              // Host header value or absolute-form host
    uint32_t hdrs_len;                        // emitted header block bytes
    uint32_t body_off, body_len;              // Content-Length span (chunked: body_len = decoded)
    uint32_t chunked;
};

// Pass 1's parse of one request, for pass 2: kind 1 = valid with its header block in emitted
// form (pass 2 only copies), kind 2 = invalid (status), kind 0 = pass 2 parses it again.
__device__ const uint8_t WIRE_SLASH[4] = {'/', 0, 0, 0};   // the "/" of a target without a path

struct WireSum {
    uint32_t kind, status, uri_len, flags;    // flags: 1 $uri verbatim, 2 chunked, minor << 8
    uint32_t method_off, method_len, target_off, target_len;
    uint32_t path_off, path_len, args_off, args_len;
    uint32_t host_off, host_len, hdr_off, hdrs_len;
    uint32_t body0, body_len, pad0, pad1;
};
static_assert(sizeof(WireSum) == 80, "WireSum layout");

__device__ __forceinline__ uint32_t wv_incl_scan(uint32_t x, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= (uint32_t)d) x += y;
    }
    return x;
}
__device__ __forceinline__ uint32_t wv_sum(uint32_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}
__device__ __forceinline__ uint32_t wv_min(uint32_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = min(x, (uint32_t)__shfl_xor(x, d));
    return x;
}
__device__ __forceinline__ uint32_t wv_max(uint32_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = max(x, (uint32_t)__shfl_xor(x, d));
    return x;
}
__device__ __forceinline__ uint32_t wv_bcast(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }

__device__ __forceinline__ bool w_upper_or(uint32_t c) { return (c - 'A' < 26u) || c == '_' || c == '-'; }
__device__ __forceinline__ bool w_alpha(uint32_t c) { return ((c | 0x20) - 'a') < 26u; }
__device__ __forceinline__ bool w_digit(uint32_t c) { return c - '0' < 10u; }
__device__ __forceinline__ bool w_alnum(uint32_t c) { return w_alpha(c) || w_digit(c); }
__device__ __forceinline__ int w_hex(uint32_t c) {
    if (w_digit(c)) return (int)(c - '0');
    c |= 0x20;
    return c - 'a' < 6u ? (int)(c - 'a' + 10) : -1;
}
__device__ __forceinline__ bool w_ieq(const uint8_t *p, uint32_t n, const char *s, uint32_t sl) {
    if (n != sl) return false;
    for (uint32_t k = 0; k < n; k++) if (lc(p[k]) != (uint32_t)(uint8_t)s[k]) return false;
    return true;
}

// ngx_http_parse_request_line over b[s0, e) (e = the line's LF), in three parts: the method and
// an absolute-form scheme / host (one lane), the request target (the whole wave: wire_target),
// the version (one lane).  Fill method, target, path, args, absolute-form host, minor; 0 or the
// HTTP status.
__device__ __forceinline__ uint32_t wire_rl_head(const uint8_t *b, uint32_t s0, uint32_t e, WireOut &o, uint32_t &t0) {
    uint32_t i = s0;
    while (i < e && w_upper_or(b[i])) i++;
    if (i == s0 || i >= e || b[i] != ' ') return 400;
    o.method_off = s0; o.method_len = i - s0;
    while (i < e && b[i] == ' ') i++;
    if (i >= e) return 400;
    t0 = i;
    if (b[i] != '/') {                                   // absolute-form
        const uint32_t sc = i;
        while (i < e && w_alpha(b[i])) i++;
        if (i == sc || i + 3 > e || b[i] != ':' || b[i + 1] != '/' || b[i + 2] != '/') return 400;
        i += 3;
        const uint32_t h0 = i;
        if (i < e && b[i] == '[') {   // sw_host_ip_literal: "[" ... "]", the brackets kept
            for (i++; i < e && b[i] != ']'; i++) {
                const uint32_t ch = b[i];
                if (w_alnum(ch)) continue;
                switch (ch) {   // unreserved and sub-delims
                case ':': case '-': case '.': case '_': case '~': case '!': case '$': case '&': case '\'':
                case '(': case ')': case '*': case '+': case ',': case ';': case '=': continue;
                default: return 400;
                }
            }
            if (i >= e) return 400;
            i++;
        } else {
            while (i < e && (w_alnum(b[i]) || b[i] == '.' || b[i] == '-')) i++;
            if (i == h0) return 400;
        }
        o.host_off = h0; o.host_len = i - h0;
        if (i < e && b[i] == ':') { i++; while (i < e && w_digit(b[i])) i++; }
        if (i >= e) return 400;
        if (b[i] != '/' && b[i] != ' ') return 400;
        t0 = i;
    }
    return 0;
}

// The target b[t0, te) by the whole wave, 16 bytes a lane per round: te = the first ' ' or '\r'
// (e if none), nul = a NUL before te, q = the first '?' or '#' before te (te if none), simple =
// the path b[t0, q) holds no '%', "//" nor "/." -- then un_one's state machine copies it verbatim.
struct WireTarget { uint32_t te, q; bool nul, simple; };
__device__ __forceinline__ WireTarget wire_target(const uint8_t *b, uint32_t t0, uint32_t e, uint32_t lane) {
    uint32_t te = GM_NONE, q = GM_NONE, z = GM_NONE, sp = GM_NONE;
    for (uint32_t r = t0; r < e && te == GM_NONE; r += 1024) {
        const uint32_t p = r + lane * 16;
        uint32_t lte = GM_NONE, lq = GM_NONE, lz = GM_NONE, lsp = GM_NONE;
        if (p < e) {
            // the lane's 16 bytes as four funnel-shifted dwords (five aligned dword reads, each
            // clamped to the last aligned dword holding a byte of the line: nothing past it is
            // read), every byte class flagged by exact SWAR compares.  Bytes past e are whatever
            // follows the line: a flag there lies at or past e >= te, which the clamps below
            // (te <= e, q <= te, nul iff z < te, simple iff sp >= q) make harmless.
            const uintptr_t ap = reinterpret_cast<uintptr_t>(b + p);
            const uint32_t sh = (uint32_t)ap & 3u;
            const uint32_t *pa = reinterpret_cast<const uint32_t *>(b + p - sh);
            const uint32_t kmax = (uint32_t)(((reinterpret_cast<uintptr_t>(b + e - 1) & ~(uintptr_t)3) - (ap - sh)) >> 2);
            uint32_t d[5];
#pragma unroll
            for (int k = 0; k < 5; k++) d[k] = pa[min((uint32_t)k, kmax)];
            uint32_t cs = p > t0 && b[p - 1] == '/' ? 0x80u : 0u;   // the byte before is a '/'
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t x = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
                const uint32_t sl = zero_bytes(x ^ 0x2F2F2F2Fu);
                const uint32_t fte = zero_bytes(x ^ 0x20202020u) | zero_bytes(x ^ 0x0D0D0D0Du);
                const uint32_t fq = zero_bytes(x ^ 0x3F3F3F3Fu) | zero_bytes(x ^ 0x23232323u);
                const uint32_t fz = zero_bytes(x);
                // '%', or "//" / "/." (a '/' before this byte: the slash flags moved up a byte)
                const uint32_t fsp = zero_bytes(x ^ 0x25252525u) | (((sl << 8) | cs) & (sl | zero_bytes(x ^ 0x2E2E2E2Eu)));
                cs = sl >> 24;
                const uint32_t at = p + 4 * k;
                if (fte && lte == GM_NONE) lte = at + ((uint32_t)__builtin_ctz(fte) >> 3);
                if (fq && lq == GM_NONE) lq = at + ((uint32_t)__builtin_ctz(fq) >> 3);
                if (fz && lz == GM_NONE) lz = at + ((uint32_t)__builtin_ctz(fz) >> 3);
                if (fsp && lsp == GM_NONE) lsp = at + ((uint32_t)__builtin_ctz(fsp) >> 3);
            }
        }
        te = wv_min(lte); q = min(q, wv_min(lq)); z = min(z, wv_min(lz)); sp = min(sp, wv_min(lsp));
    }
    WireTarget t;
    t.te = min(te, e);
    t.q = min(q, t.te);
    t.nul = z < t.te;
    t.simple = sp >= t.q;
    return t;
}

__device__ __forceinline__ uint32_t wire_rl_tail(const uint8_t *b, uint32_t e, uint32_t t0, const WireTarget &tg, WireOut &o) {
    const uint32_t te = tg.te;
    if (tg.nul) return 400;
    if (te >= e || b[te] != ' ') return 400;              // HTTP/0.9 (no version)
    o.args_off = 0; o.args_len = 0;
    if (te == t0) { o.target_off = o.path_off = GM_NONE; o.target_len = o.path_len = 1; }   // "/"
    else {
        o.target_off = t0; o.target_len = te - t0;
        o.path_off = t0; o.path_len = tg.q - t0;
        if (tg.q < te && b[tg.q] == '?') { o.args_off = tg.q + 1; o.args_len = te - tg.q - 1; }
    }
    uint32_t i = te;
    while (i < e && b[i] == ' ') i++;
    if (i + 5 > e || b[i] != 'H' || b[i + 1] != 'T' || b[i + 2] != 'T' || b[i + 3] != 'P' || b[i + 4] != '/') return 400;
    i += 5;
    uint32_t major = 0, minor = 0, d0 = i;
    while (i < e && w_digit(b[i])) { major = major * 10 + (b[i] - '0'); if (major > 99) return 400; i++; }
    if (i == d0 || i >= e || b[i] != '.') return 400;
    i++; d0 = i;
    while (i < e && w_digit(b[i])) { minor = minor * 10 + (b[i] - '0'); if (minor > 99) return 400; i++; }
    if (i == d0) return 400;
    while (i < e && b[i] == ' ') i++;
    if (i < e && b[i] == '\r') i++;
    if (i != e) return 400;
    if (major > 1) return 505;
    if (major < 1) return 400;
    o.minor = minor;
    return 0;
}

// one chunk-size line at b[i..): the chunk's data offset and size (0 = last chunk, then the
// trailer up to its empty line is consumed: *next = after it); false = malformed
__device__ bool wire_chunk(const uint8_t *b, uint32_t n, uint32_t &i, uint32_t &data, uint64_t &size) {
    uint64_t sz = 0;
    const uint32_t d0 = i;
    int v;
    while (i < n && (v = w_hex(b[i])) >= 0) {
        if (sz > (0x7FFFFFFFFFFFFFFFull >> 4) - 1) return false;
        sz = sz * 16 + (uint32_t)v;
        i++;
    }
    if (i == d0 || i >= n) return false;
    if (b[i] == '\r') { i++; if (i >= n || b[i] != '\n') return false; }
    else if (b[i] == ';' || b[i] == ' ' || b[i] == '\t') { while (i < n && b[i] != '\n') i++; if (i >= n) return false; }
    else if (b[i] != '\n') return false;
    i++;
    data = i;
    size = sz;
    if (sz == 0) {   // trailer lines up to the empty line
        for (;;) {
            if (i >= n) return false;
            uint32_t e = i;
            while (e < n && b[e] != '\n') e++;
            if (e >= n) return false;
            uint32_t le = e;
            if (le > i && b[le - 1] == '\r') le--;
            const bool empty = le == i;
            i = e + 1;
            if (empty) return true;
        }
    }
    if ((uint64_t)(n - i) < sz) return false;
    i += (uint32_t)sz;
    if (i < n && b[i] == '\r') i++;
    if (i >= n || b[i] != '\n') return false;
    i++;
    return true;
}

// one lane's copy of n bytes, any alignments: bytes up to a 4-aligned destination, then dwords
// funnel-shifted from the two aligned source dwords that hold them (the second starts inside
// the source span, so nothing past its last aligned dword is read), then the tail bytes
__device__ __forceinline__ void lane_copy(uint8_t *dst, const uint8_t *src, uint32_t n) {
    uint32_t k = 0;
    while (k < n && ((uintptr_t)(dst + k) & 3)) { dst[k] = src[k]; k++; }
    for (; k + 4 <= n; k += 4) {
        const uint8_t *sp = src + k;
        const uint32_t sh = (uint32_t)((uintptr_t)sp & 3);
        const uint32_t *a = reinterpret_cast<const uint32_t *>(sp - sh);
        const uint32_t lo = a[0], hi = sh ? a[1] : 0u;
        *reinterpret_cast<uint32_t *>(dst + k) = __builtin_amdgcn_alignbyte(hi, lo, sh);
    }
    for (; k < n; k++) dst[k] = src[k];
}
// n bytes src -> dst, any alignments (src in LDS or global memory), by the whole wave: the
// destination in 16-byte aligned chunks, a lane per chunk, each chunk from five funnel-shifted
// source dwords; the bytes before the first and after the last chunk byte by byte.  A chunk
// whose dword reads would pass src + n (the last) is read byte by byte too.
__device__ void wave_copy(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane) {
    const uint32_t head = min(n, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15));
    if (lane < head) dst[lane] = src[lane];
    const uint32_t nb = (n - head) >> 4;
    const uint8_t *s = src + head;
    uint8_t *d = dst + head;
    for (uint32_t c = lane; c < nb; c += 64) {
        const uint8_t *sp = s + 16 * c;
        const uint32_t sh = (uint32_t)((uintptr_t)sp & 3);
        uint32_t q[5];
        if (head + 16 * c + 20 <= n + sh) {
            const uint32_t *a = reinterpret_cast<const uint32_t *>(sp - sh);
#pragma unroll
            for (int k = 0; k < 5; k++) q[k] = a[k];
        } else {
#pragma unroll
            for (int k = 0; k < 5; k++) {
                q[k] = 0;
                for (int bb = 0; bb < 4; bb++) {
                    const int o = 4 * k + bb - (int)sh;   // byte of sp
                    if (o >= 0 && o < 16) q[k] |= (uint32_t)sp[o] << (8 * bb);
                }
            }
        }
        uint4 v;
        v.x = __builtin_amdgcn_alignbyte(q[1], q[0], sh); v.y = __builtin_amdgcn_alignbyte(q[2], q[1], sh);
        v.z = __builtin_amdgcn_alignbyte(q[3], q[2], sh); v.w = __builtin_amdgcn_alignbyte(q[4], q[3], sh);
        *reinterpret_cast<uint4 *>(d + 16 * c) = v;
    }
    for (uint32_t k = head + 16 * nb + lane; k < n; k += 64) dst[k] = src[k];
}

// one header line t (1 <= t < L) of the table: name / value bounds, validity, length.  Scans
// only to the first ':' (aligned dwords between byte-wise ends), checking the name's bytes on the
// way -- a NUL anywhere in the header lines is found once per message by the line-table pass.
struct WireLine { uint32_t ns, nlen, vs, ve, olen; bool valid, toolong; };
__device__ __forceinline__ bool w_name_ch(uint32_t ch) { return w_alnum(ch) || ch == '-'; }
// bit 7 of each byte of x that is not a header-name character (w_name_ch: [A-Za-z0-9-]), by SWAR
// range tests on the low seven bits (no carry leaves a byte: each sum stays below 0x100)
__device__ __forceinline__ uint32_t name_bad(uint32_t x) {
    const uint32_t y = x & 0x7F7F7F7Fu, l = y | 0x20202020u;
    const uint32_t alpha = (l + 0x1F1F1F1Fu) & ~(l + 0x05050505u);   // 'a' <= l <= 'z'
    const uint32_t digit = (y + 0x50505050u) & ~(y + 0x46464646u);   // '0' <= y <= '9'
    const uint32_t ok = (alpha | digit | zero_bytes(x ^ 0x2D2D2D2Du)) & ~x;   // (a set bit 7: not ASCII)
    return ~ok & 0x80808080u;
}
__device__ __forceinline__ WireLine wire_line(const uint8_t *b, const uint32_t *tab, uint32_t t) {
    WireLine w{};
    const uint32_t st = tab[t - 1] + 1, e = tab[t];
    uint32_t le = e;
    if (le > st && b[le - 1] == '\r') le--;
    w.toolong = e + 1 - st > 8192;
    uint32_t c = le;
    bool ok = true;
    for (uint32_t k = st; k < le && c == le;) {
        if (((uintptr_t)(b + k) & 3) == 0 && k + 4 <= le) {
            const uint32_t x = *reinterpret_cast<const uint32_t *>(b + k);
            const uint32_t zc = zero_bytes(x ^ 0x3A3A3A3Au);
            const uint32_t nb = zc ? (uint32_t)__builtin_ctz(zc) >> 3 : 4u;   // name bytes in x
            ok &= (name_bad(x) & (nb >= 4 ? 0xFFFFFFFFu : (1u << (8 * nb)) - 1u)) == 0;
            if (zc) c = k + nb;
            k += 4;
        } else {
            const uint32_t ch = b[k];
            if (ch == ':') c = k; else ok &= w_name_ch(ch);
            k++;
        }
    }
    w.ns = st; w.nlen = c - st;
    w.vs = c < le ? c + 1 : le;
    while (w.vs < le && b[w.vs] == ' ') w.vs++;
    w.ve = le;
    while (w.ve > w.vs && b[w.ve - 1] == ' ') w.ve--;
    w.valid = w.nlen > 0 && ok;
    w.olen = w.valid ? w.nlen + 2 + (w.ve - w.vs) + 2 : 0;
    return w;
}

// One request, one wave (every branch below is wave-uniform: per-lane results meet in wave
// reductions / broadcasts).  EMIT = false: returns the record's exact slot size (16-B aligned);
// EMIT = true: writes the fields at base, zero-fills the rest of the slot, writes the gm_req.
// `scr` (the wave's 8 KiB in global memory, WIRE_SCR) receives the $uri (the request line is
// <= 8 KiB, else 414; in LDS it capped a CU at 16 of these waves, latency-bound on lane-serial
// phases, where 32 now fit); the emit pass
// copies it out only once the request is known valid -- written straight into the arena, a
// request found invalid later (a bad escape mid-path, a header error) would have spilled its path
// over the next request's slot (its own slot then holds only $remote_addr).
template <bool EMIT>
__device__ __forceinline__ uint64_t wire_one(const uint8_t *__restrict__ W, const gm_wire_msg &m, uint32_t *tab, uint8_t *scr,
                             uint8_t *stg, uint32_t lane, uint8_t *__restrict__ out, uint64_t base, uint64_t slot,
                             gm_req *rec, WireSum *sum, uint32_t fmask, uint32_t *kf = nullptr,
                             uint2 *pieces = nullptr) {
    uint32_t npieces = 0;   // (lane 0) chunks of a chunked body
    const uint8_t *b = W + m.off;
    const uint32_t n = m.len;
    const uint32_t ra = min((uint32_t)m.raddr_len, 40u);
    const uint32_t mf = m.flags & fmask;   // (the WIRE_F_* bits count only when k_wire_proxy ran)
    const uint32_t pa = (mf & WIRE_F_PADDR) ? min((uint32_t)m.paddr_len, PADDR_MAX) : 0u;
    uint32_t status = (mf & WIRE_F_BROKEN) ? 444u : 0u;   // a broken PROXY header: closed
    if (EMIT && slot == 0) {   // past the arena's capacity (a void batch): an empty invalid record
        if (lane == 0) {
            gm_req r = {};
            r.base = base;
            r.port = m.port; r.remote_port = m.remote_port;
            r.flags = (m.flags & (GM_REQ_HTTPS | GM_REQ_HTTP2)) | GM_REQ_INVALID;
            r.pad0[1] = 500 & 0xFF; r.pad0[2] = 500 >> 8;
            *rec = r;
        }
        return 0;
    }
    // ---- leading CR / LF (lane 0), then the line table up to the empty line
    uint32_t s0 = 0;
    if (lane == 0) while (s0 < n && (b[s0] == '\r' || b[s0] == '\n')) s0++;
    s0 = wv_bcast(s0);
    uint32_t nl = 0, L = GM_NONE;           // lines recorded, index of the empty line
    uint32_t first_nul = GM_NONE;           // the first NUL byte scanned (message offset)
    // windows from the message start (not s0), so that the first WIRE_STAGE bytes land in the
    // wave's LDS stage at their own offsets; LFs before s0 (leading blank lines) are masked
    for (uint32_t w = 0; w < n && L == GM_NONE && status == 0; w += 1024) {
        // the lane's 16 bytes: five funnel-shifted dword loads (bytes at or past n read as 0 and
        // are masked), LFs flagged by an exact SWAR byte compare
        const uint32_t p = w + lane * 16;
        uint32_t mask = 0, lnul = GM_NONE;
        uint32_t v[4] = {0, 0, 0, 0};
        if (p < n) {
            const uint32_t sh = (uint32_t)((uintptr_t)(b + p) & 3);
            uint32_t q[5];
            // five aligned dwords, each clamped to the last dword that holds a message byte (an
            // aligned dword never crosses a page, so one holding a valid byte is always readable):
            // no byte-wise path at the message's end (20 dependent byte loads in their own
            // branches, once per message); bytes at or past n are zeroed below
            const uint32_t *a = reinterpret_cast<const uint32_t *>(b + p - sh);
            const uint32_t kmax = (n - 1 - (p - sh)) >> 2;   // the last dword index inside [0, n)
#pragma unroll
            for (int k = 0; k < 5; k++) q[k] = a[min((uint32_t)k, kmax)];
            const uint32_t rem = n - p;   // valid bytes from p (>= 1)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                v[k] = __builtin_amdgcn_alignbyte(q[k + 1], q[k], sh);
                const uint32_t vb = rem > 4u * k ? min(rem - 4u * k, 4u) : 0u;
                v[k] &= vb >= 4 ? 0xFFFFFFFFu : (1u << (8 * vb)) - 1u;
                const uint32_t z = zero_bytes(v[k] ^ 0x0A0A0A0Au);
                mask |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * k);
                // NUL bytes among the valid ones (the bytes past n were zeroed above)
                const uint32_t zn = zero_bytes(v[k]) & (vb >= 4 ? 0xFFFFFFFFu : (1u << (8 * vb)) - 1u);
                if (zn && lnul == GM_NONE) lnul = p + 4 * k + ((uint32_t)__builtin_ctz(zn) >> 3);
            }
            if (n - p < 16) mask &= (1u << (n - p)) - 1u;   // (a zero byte past n is not an LF)
            if (s0 > p) mask &= s0 - p >= 16 ? 0u : ~((1u << (s0 - p)) - 1u);
        }
        if (p + 16 <= WIRE_STAGE) reinterpret_cast<uint4 *>(stg)[p >> 4] = make_uint4(v[0], v[1], v[2], v[3]);
        first_nul = min(first_nul, wv_min(lnul));
        const uint32_t c = __popc(mask), incl = wv_incl_scan(c, lane), tot = __shfl(incl, 63);
        uint32_t si = nl + incl - c;
        for (uint32_t mm = mask; mm; mm &= mm - 1, si++)
            if (si < WIRE_LINES) tab[si] = w + lane * 16 + (uint32_t)(__ffs(mm) - 1);
        __builtin_amdgcn_wave_barrier();
        const uint32_t lim = min(nl + tot, WIRE_LINES);
        uint32_t first = GM_NONE;
        for (uint32_t t = nl + lane; t < lim; t += 64) {
            if (t == 0) continue;             // the request line is never empty (s0 skipped CR / LF)
            const uint32_t st = tab[t - 1] + 1, e = tab[t];
            if (e == st || (e == st + 1 && (st < WIRE_STAGE ? stg[st] : b[st]) == '\r')) first = min(first, t);
        }
        first = wv_min(first);
        nl = lim;
        if (first != GM_NONE) L = first;
        else if (nl >= WIRE_LINES) status = 400;   // more header lines than the table holds
        __builtin_amdgcn_wave_barrier();
    }
    // the header as staged in LDS (the usual case: the line table ends inside the stage), else
    // global memory -- every lane-serial parse below reads it.  The rest of the parse is written
    // once and inlined twice, so that the staged copy reads the header with LDS instructions: through
    // one pointer that may be either, every byte read was a flat load (memory latency and both
    // counters; 57 flat byte loads in the size pass, no LDS read).
    __builtin_amdgcn_wave_barrier();
    auto rest = [&](const uint8_t *hb) __attribute__((always_inline)) -> uint64_t {
        // ---- the request line (lane 0) and its $uri: 414 / 400 / 505, then the complex URI
        WireOut o = {};
        if (nl > 0 && tab[0] + 1 - s0 > 8192) status = 414;
        else if (status == 0 && L == GM_NONE) status = 400;    // no empty line: incomplete header
        uint32_t uri_len = 0;
        bool uri_direct = false;                  // $uri = the path's bytes as they are (no scratch copy)
        if (status == 0) {
            uint32_t rs = 0, ul = 0, t0 = 0;
            if (lane == 0) rs = wire_rl_head(hb, s0, tab[0], o, t0);
            rs = wv_bcast(rs);
            t0 = wv_bcast(t0);
            WireTarget tg{};
            if (rs == 0) tg = wire_target(hb, t0, tab[0], lane);
            uri_direct = rs == 0 && tg.simple;
            if (lane == 0 && rs == 0) {
                rs = wire_rl_tail(hb, tab[0], t0, tg, o);
                if (rs == 0) {
                    if (o.path_off == GM_NONE) { scr[0] = '/'; ul = 1; uri_direct = false; }
                    else if (uri_direct) ul = o.path_len;
                    else ul = un_one(hb + o.path_off, o.path_len, scr);
                    if (ul == GM_NONE) rs = 400;
                }
            }
            uri_direct = wv_bcast(uri_direct ? 1u : 0u) != 0;
            status = wv_bcast(rs);
            uri_len = wv_bcast(ul);
            o.path_off = wv_bcast(o.path_off);
            o.minor = wv_bcast(o.minor);
            o.method_off = wv_bcast(o.method_off); o.method_len = wv_bcast(o.method_len);
            o.target_off = wv_bcast(o.target_off); o.target_len = wv_bcast(o.target_len);
            o.args_off = wv_bcast(o.args_off); o.args_len = wv_bcast(o.args_len);
            o.host_off = wv_bcast(o.host_off); o.host_len = wv_bcast(o.host_len);   // absolute-form host
        }
        // ---- header lines 1 .. L-1, a lane per line (rounds of 64)
        uint32_t hdrs_len = 0, te_kind = 0;
        uint64_t cl = 0;
        bool have_host = false;
        // every header line already in its emitted form "name: value\r\n" (a valid name, one space
        // after the ':', none after the value, CRLF): the header block is then the input's bytes
        // from line 1 to the empty line, one wave copy
        uint32_t noncanon = 0;
        if (status == 0) {
            uint32_t n_host = 0, n_cl = 0, bad = 0, cl_bad = 0;
            uint32_t my_host = GM_NONE, my_hvs = 0, my_hvl = 0, my_te = GM_NONE, my_tek = 0, my_cl = GM_NONE;
            uint64_t my_clv = 0;
            for (uint32_t r0 = 1; r0 < L; r0 += 64) {
                const uint32_t t = r0 + lane;
                uint32_t olen = 0;
                if (t < L) {
                    const WireLine w = wire_line(hb, tab, t);
                    bad |= w.toolong ? 1u : 0u;
                    olen = w.olen;
                    noncanon |= (w.valid && w.vs == w.ns + w.nlen + 2 && w.ve == tab[t] - 1 && hb[w.ve] == '\r') ? 0u : 1u;
                    if (w.valid) {
                        const uint8_t *nm = hb + w.ns;
                        if (w_ieq(nm, w.nlen, "host", 4)) {
                            n_host++;
                            if (my_host == GM_NONE) { my_host = t; my_hvs = w.vs; my_hvl = w.ve - w.vs; }
                        } else if (w_ieq(nm, w.nlen, "content-length", 14)) {
                            n_cl++;
                            if (my_cl == GM_NONE) {
                                my_cl = t;
                                uint64_t v = 0;
                                if (w.ve == w.vs) cl_bad = 1;
                                for (uint32_t k = w.vs; k < w.ve && !cl_bad; k++) {
                                    const uint32_t ch = hb[k];
                                    if (!w_digit(ch) || v > (0x7FFFFFFFFFFFFFFFull - 9) / 10) cl_bad = 1;
                                    else v = v * 10 + (ch - '0');
                                }
                                my_clv = v;
                            }
                        } else if (w_ieq(nm, w.nlen, "transfer-encoding", 17) && my_te == GM_NONE) {
                            my_te = t;
                            my_tek = w_ieq(hb + w.vs, w.ve - w.vs, "chunked", 7) ? 1u
                                     : w_ieq(hb + w.vs, w.ve - w.vs, "identity", 8) ? 2u : 3u;
                        }
                    }
                }
                hdrs_len += wv_sum(olen);
            }
            n_host = wv_sum(n_host); n_cl = wv_sum(n_cl); bad = wv_max(bad); noncanon = wv_max(noncanon);
            if (first_nul < tab[L]) bad = 1;   // a NUL in a header line (one in the request line: 400 above)
            // line-level errors (NUL, over-long line, a second Host / Content-Length)
            if (bad || n_host > 1 || n_cl > 1) status = 400;
            else if (n_host == 0 && o.minor >= 1) status = 400;     // HTTP/1.1 without Host
            else {
                if (n_cl == 1) {
                    const uint32_t src = wv_min(my_cl != GM_NONE ? lane : 64u);
                    if (__shfl(cl_bad, (int)src)) status = 400;
                    cl = ((uint64_t)__shfl((uint32_t)(my_clv >> 32), (int)src) << 32) | __shfl((uint32_t)my_clv, (int)src);
                }
                const uint32_t te_line = wv_min(my_te);
                if (status == 0 && te_line != GM_NONE) {
                    te_kind = __shfl(my_tek, (int)wv_min(my_te == te_line ? lane : 64u));
                    if (te_kind == 3) status = 501;
                }
                if (n_host == 1 && o.host_len == 0) {                // no absolute-form host: the header's
                    const uint32_t src = wv_min(my_host != GM_NONE ? lane : 64u);
                    o.host_off = __shfl(my_hvs, (int)src);
                    o.host_len = __shfl(my_hvl, (int)src);
                }
                have_host = n_host == 1 || o.host_len > 0;
            }
        }
        (void)have_host;
        // ---- body: chunked (lane 0 walks the chunk lines) or Content-Length
        const uint32_t body0 = status == 0 ? tab[L] + 1 : 0;
        uint64_t body_len = 0;
        const bool chunked = status == 0 && te_kind == 1;
        if (status == 0) {
            if (chunked) {
                uint32_t ok = 1;
                uint64_t tot = 0;
                if (lane == 0) {
                    uint32_t i = body0, data, np = 0;
                    uint64_t sz;
                    for (;;) {
                        if (!wire_chunk(b, n, i, data, sz)) { ok = 0; break; }
                        if (sz == 0) break;
                        // the first WIRE_PIECES chunks' spans, for pass 2's flat gather
                        if (pieces && np < WIRE_PIECES) pieces[np] = make_uint2(data, (uint32_t)sz);
                        np++;
                        tot += sz;
                    }
                    npieces = np;
                }
                ok = wv_bcast(ok);
                body_len = ((uint64_t)wv_bcast((uint32_t)(tot >> 32)) << 32) | wv_bcast((uint32_t)tot);
                if (!ok || body_len > 0xFFFFFFFFull) status = 400;
            } else if (cl) {
                if ((uint64_t)(n - body0) < cl) status = 400;
                else body_len = cl;
            }
        }
        // The size is built with an `if`, not `okreq ? (u64 sum) : (u32) ra`: that select form gave
        // sizes whose upper dword held the status (measured on the GPU with scripts/dbg_wire.py, hipcc
        // 7.2; the if form gives the oracle's sizes).  status is wave-uniform by construction (every
        // update above is a reduction or a broadcast); the broadcast states it.
        status = wv_bcast(status);
        const bool okreq = status == 0;
        uint64_t tot = ra + pa;
        if (okreq) tot += (uint64_t)uri_len + o.args_len + hdrs_len + body_len + o.host_len + o.method_len + o.target_len;
        const uint64_t need = (tot + 15) & ~15ull;
        if (!EMIT) {
            if (lane == 0) {
                WireSum q = {};
                q.kind = !okreq ? 2u : (GM_WIRE_CANON && !noncanon) ? 1u : 0u;
                q.status = status;
                q.uri_len = uri_len;
                q.flags = (uri_direct ? 1u : 0u) | (chunked ? 2u : 0u) | o.minor << 8;
                q.method_off = o.method_off; q.method_len = o.method_len;
                q.target_off = o.target_off; q.target_len = o.target_len;
                q.path_off = o.path_off; q.path_len = o.path_len;
                q.args_off = o.args_off; q.args_len = o.args_len;
                q.host_off = o.host_off; q.host_len = o.host_len;
                q.hdr_off = okreq ? tab[0] + 1 : 0; q.hdrs_len = hdrs_len;
                q.body0 = body0; q.body_len = (uint32_t)body_len;
                q.pad0 = chunked ? npieces : 0u;   // pieces recorded: min(pad0, WIRE_PIECES)
                *sum = q;
                if (kf) *kf = q.kind | q.flags << 8 | (chunked && npieces > WIRE_PIECES ? 1u << 31 : 0u);
            }
            return need;
        }
        // ---- emit at base: uri (already written by lane 0) | args | hdrs | body | host | method | ruri | raddr
        uint32_t st_final = status;
        if (need > slot) st_final = 500;   // arena capacity exceeded (the batch is void, gm_sync says so)
        uint64_t p = base;
        uint32_t lens[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (st_final == 0) {
            __threadfence_block();              // lane 0's $uri stores in scr, visible to the wave
            __builtin_amdgcn_wave_barrier();
            wave_copy(out + p, uri_direct ? hb + o.path_off : scr, uri_len, lane);
            p += uri_len;
            wave_copy(out + p, hb + o.args_off, o.args_len, lane);
            p += o.args_len;
            if (GM_WIRE_CANON && !noncanon) {
                wave_copy(out + p, hb + tab[0] + 1, hdrs_len, lane);
                p += hdrs_len;
            }
            else for (uint32_t r0 = 1; r0 < L; r0 += 64) {   // header lines at wave-prefix offsets
                const uint32_t t = r0 + lane;
                WireLine w{};
                if (t < L) w = wire_line(hb, tab, t);
                const uint32_t incl = wv_incl_scan(w.olen, lane);
                if (w.olen) {
                    uint8_t *q = out + p + (incl - w.olen);
                    lane_copy(q, hb + w.ns, w.nlen);
                    q[w.nlen] = ':'; q[w.nlen + 1] = ' ';
                    lane_copy(q + w.nlen + 2, hb + w.vs, w.ve - w.vs);
                    q[w.olen - 2] = '\r'; q[w.olen - 1] = '\n';
                }
                p += __shfl(incl, 63);
            }
            if (chunked) {
                uint32_t i = body0;
                for (;;) {
                    uint32_t data = 0, last = 0;
                    uint64_t sz = 0;
                    if (lane == 0) {
                        wire_chunk(b, n, i, data, sz);   // validated by the size pass
                        last = sz == 0;
                    }
                    if (wv_bcast(last)) break;
                    data = wv_bcast(data);
                    const uint32_t s32 = wv_bcast((uint32_t)sz);
                    wave_copy(out + p, b + data, s32, lane);
                    p += s32;
                    i = wv_bcast(i);
                }
            } else {
                wave_copy(out + p, b + body0, (uint32_t)body_len, lane);
                p += body_len;
            }
            wave_copy(out + p, hb + o.host_off, o.host_len, lane); p += o.host_len;
            wave_copy(out + p, hb + o.method_off, o.method_len, lane); p += o.method_len;
            if (o.target_off == GM_NONE) { if (lane == 0) out[p] = '/'; }
            else wave_copy(out + p, hb + o.target_off, o.target_len, lane);
            p += o.target_len;
            lens[0] = uri_len; lens[1] = o.args_len; lens[2] = hdrs_len; lens[3] = (uint32_t)body_len;
            lens[4] = o.host_len; lens[5] = o.method_len; lens[6] = o.target_len;
        }
        uint32_t pl = 0;
        if (ra + pa <= base + slot - p) {
            wave_copy(out + p, m.raddr, ra, lane);
            p += ra;
            lens[7] = ra;
            wave_copy(out + p, m.paddr, pa, lane);
            p += pa;
            pl = pa;
        }
        for (uint64_t k = p + lane; k < base + slot; k += 64) out[k] = 0;   // the slot's tail (alignment)
        if (lane == 0) {
            gm_req r = {};
            r.base = base;
            r.uri_len = lens[0]; r.args_len = lens[1]; r.hdr_len = lens[2]; r.body_len = lens[3];
            r.host_len = (uint16_t)lens[4]; r.method_len = (uint16_t)lens[5]; r.ruri_len = (uint16_t)lens[6];
            r.raddr_len = (uint16_t)lens[7];
            r.port = m.port; r.remote_port = m.remote_port;
            r.flags = m.flags & (GM_REQ_HTTPS | GM_REQ_HTTP2);
            r.pad0[0] = (uint8_t)pl;
            if (pl) { r.pad1[0] = (uint8_t)m.proxy_port; r.pad1[1] = (uint8_t)(m.proxy_port >> 8); }
            if (st_final) { r.flags |= GM_REQ_INVALID; r.pad0[1] = (uint8_t)st_final; r.pad0[2] = (uint8_t)(st_final >> 8); }
            else {
                if (o.minor == 0) r.flags |= GM_REQ_HTTP10;
                if (chunked) r.flags |= GM_REQ_CHUNKED;
            }
            for (int k = 0; k < 16; k++) r.rid[k] = m.rid[k];
            *rec = r;
        }
        return need;
    };
    if (L != GM_NONE && tab[L] < WIRE_STAGE) return rest(stg);
    return rest(b);
}

// The slot [dst, dst + slot) as the concatenation of 8 source segments, zero past their total
// (dst 16-byte aligned, slot a multiple of 16): a lane per 16-byte output chunk, every chunk's
// loads issued before any store.  A chunk inside one segment is five funnel-shifted dwords (when
// they stay inside the segment's aligned span), any other chunk 16 byte gathers.
struct WireSegs { const uint8_t *p[9]; uint32_t end[9]; };   // end = prefix sum of the lengths
__device__ __forceinline__ void wire_seg_of(const WireSegs &g, uint32_t o, const uint8_t *&sp, uint32_t &st,
                                            uint32_t &en) {
    sp = g.p[8]; st = g.end[7]; en = g.end[8];
#pragma unroll
    for (int k = 7; k >= 0; k--) {
        const bool in = o < g.end[k];
        sp = in ? g.p[k] : sp;
        en = in ? g.end[k] : en;
        st = in ? (k ? g.end[k - 1] : 0u) : st;
    }
}
__device__ void wire_gather(uint8_t *__restrict__ dst, const WireSegs &g, uint32_t slot, uint32_t lane) {
    const uint32_t total = g.end[8];
    for (uint32_t o0 = lane * 16; o0 < slot; o0 += 1024) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (o0 < total) {
            const uint8_t *sp; uint32_t st, en;
            wire_seg_of(g, o0, sp, st, en);
            const uint8_t *src = sp + (o0 - st);
            const uint32_t sh = (uint32_t)((uintptr_t)src & 3);
            if (o0 + 16 <= en && (o0 - st) + 20 <= (en - st) + sh) {
                const uint32_t *a = reinterpret_cast<const uint32_t *>(src - sh);
                uint32_t q[5];
#pragma unroll
                for (int k = 0; k < 5; k++) q[k] = a[k];
                v.x = __builtin_amdgcn_alignbyte(q[1], q[0], sh); v.y = __builtin_amdgcn_alignbyte(q[2], q[1], sh);
                v.z = __builtin_amdgcn_alignbyte(q[3], q[2], sh); v.w = __builtin_amdgcn_alignbyte(q[4], q[3], sh);
            } else {
                // a chunk across segment ends: 16 byte loads, all issued before any is used (a
                // byte past the total reads segment 0's first byte and is dropped)
                uint32_t ch[16];
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const uint32_t o = o0 + j;
                    const uint8_t *bp; uint32_t bs, be;
                    const uint32_t oc = min(o, total - 1);
                    wire_seg_of(g, oc, bp, bs, be);
                    const uint32_t x = bp[oc - bs];   // (unconditional: always a valid byte)
                    ch[j] = o < total ? x : 0u;
                }
                uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < 16; j++) w[j >> 2] |= ch[j] << (8 * (j & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        *reinterpret_cast<uint4 *>(dst + o0) = v;
    }
}

// Pass 2 from pass 1's summary (kind 1 or 2): the copies only -- the same bytes and record as
// wire_one<true> writes for the request (kind 1: the header block is the input span).
// GATHER: the caller knows the request is kind 1 without a chunked body (the one-gather form).
template <bool GATHER>
__device__ void wire_emit_sum(const uint8_t *__restrict__ W, const gm_wire_msg &m, const WireSum &sm, uint8_t *scr,
                              uint32_t lane, uint8_t *__restrict__ out, uint64_t base, uint64_t slot, gm_req *rec,
                              uint32_t fmask) {
    const uint8_t *b = W + m.off;
    const uint32_t ra = min((uint32_t)m.raddr_len, 40u);
    const uint32_t pa = ((m.flags & fmask) & WIRE_F_PADDR) ? min((uint32_t)m.paddr_len, PADDR_MAX) : 0u;
    const uint32_t kind = wv_bcast(sm.kind), flags = wv_bcast(sm.flags);
    uint64_t p = base;
    uint32_t lens[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t pl = 0;
    if (GATHER || (kind == 1 && !(flags & 2u))) {         // one gather: uri | args | hdrs | body | host | method | ruri | raddr
        const uint32_t path_off = wv_bcast(sm.path_off), target_off = wv_bcast(sm.target_off);
        WireSegs g;
        lens[0] = wv_bcast(sm.uri_len); lens[1] = wv_bcast(sm.args_len); lens[2] = wv_bcast(sm.hdrs_len);
        lens[3] = wv_bcast(sm.body_len); lens[4] = wv_bcast(sm.host_len); lens[5] = wv_bcast(sm.method_len);
        lens[6] = wv_bcast(sm.target_len); lens[7] = ra;
        if (path_off == GM_NONE) g.p[0] = reinterpret_cast<const uint8_t *>(WIRE_SLASH);
        else if (flags & 1u) g.p[0] = b + path_off;
        else {
            if (lane == 0) (void)un_one(b + path_off, wv_bcast(sm.path_len), scr);
            __threadfence_block();
            __builtin_amdgcn_wave_barrier();
            g.p[0] = scr;
        }
        g.p[1] = b + wv_bcast(sm.args_off); g.p[2] = b + wv_bcast(sm.hdr_off); g.p[3] = b + wv_bcast(sm.body0);
        g.p[4] = b + wv_bcast(sm.host_off); g.p[5] = b + wv_bcast(sm.method_off);
        g.p[6] = target_off == GM_NONE ? reinterpret_cast<const uint8_t *>(WIRE_SLASH) : b + target_off;
        g.p[7] = m.raddr;
        g.p[8] = m.paddr;
        uint32_t e = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) { e += lens[k]; g.end[k] = e; }
        g.end[8] = e + pa;
        pl = pa;
        wire_gather(out + base, g, (uint32_t)slot, lane);
    } else if (!GATHER && kind == 1) {
        const uint32_t uri_len = wv_bcast(sm.uri_len), path_off = wv_bcast(sm.path_off);
        if (path_off == GM_NONE) { if (lane == 0) out[p] = '/'; }
        else if (flags & 1u) wave_copy(out + p, b + path_off, uri_len, lane);
        else {
            if (lane == 0) (void)un_one(b + path_off, wv_bcast(sm.path_len), scr);
            __threadfence_block();
            __builtin_amdgcn_wave_barrier();
            wave_copy(out + p, scr, uri_len, lane);
        }
        p += uri_len;
        const uint32_t args_len = wv_bcast(sm.args_len), hdrs_len = wv_bcast(sm.hdrs_len);
        wave_copy(out + p, b + wv_bcast(sm.args_off), args_len, lane); p += args_len;
        wave_copy(out + p, b + wv_bcast(sm.hdr_off), hdrs_len, lane); p += hdrs_len;
        const uint32_t body0 = wv_bcast(sm.body0), body_len = wv_bcast(sm.body_len);
        if (flags & 2u) {
            const uint32_t n = m.len;
            uint32_t i = body0;
            for (;;) {
                uint32_t data = 0, last = 0;
                uint64_t sz = 0;
                if (lane == 0) {
                    wire_chunk(b, n, i, data, sz);   // validated by the size pass
                    last = sz == 0;
                }
                if (wv_bcast(last)) break;
                data = wv_bcast(data);
                const uint32_t s32 = wv_bcast((uint32_t)sz);
                wave_copy(out + p, b + data, s32, lane);
                p += s32;
                i = wv_bcast(i);
            }
        } else {
            wave_copy(out + p, b + body0, body_len, lane);
            p += body_len;
        }
        const uint32_t host_len = wv_bcast(sm.host_len), method_len = wv_bcast(sm.method_len);
        const uint32_t target_off = wv_bcast(sm.target_off), target_len = wv_bcast(sm.target_len);
        wave_copy(out + p, b + wv_bcast(sm.host_off), host_len, lane); p += host_len;
        wave_copy(out + p, b + wv_bcast(sm.method_off), method_len, lane); p += method_len;
        if (target_off == GM_NONE) { if (lane == 0) out[p] = '/'; }
        else wave_copy(out + p, b + target_off, target_len, lane);
        p += target_len;
        lens[0] = uri_len; lens[1] = args_len; lens[2] = hdrs_len; lens[3] = body_len;
        lens[4] = host_len; lens[5] = method_len; lens[6] = target_len;
    }
    if (!GATHER && !(kind == 1 && !(flags & 2u))) {
        if (ra + pa <= base + slot - p) {
            wave_copy(out + p, m.raddr, ra, lane);
            p += ra;
            lens[7] = ra;
            wave_copy(out + p, m.paddr, pa, lane);
            p += pa;
            pl = pa;
        }
        for (uint64_t k = p + lane; k < base + slot; k += 64) out[k] = 0;   // the slot's tail (alignment)
    }
    if (lane == 0) {
        const uint32_t st = kind == 2 ? sm.status : 0u;
        gm_req r = {};
        r.base = base;
        r.uri_len = lens[0]; r.args_len = lens[1]; r.hdr_len = lens[2]; r.body_len = lens[3];
        r.host_len = (uint16_t)lens[4]; r.method_len = (uint16_t)lens[5]; r.ruri_len = (uint16_t)lens[6];
        r.raddr_len = (uint16_t)lens[7];
        r.port = m.port; r.remote_port = m.remote_port;
        r.flags = m.flags & (GM_REQ_HTTPS | GM_REQ_HTTP2);
        r.pad0[0] = (uint8_t)pl;
        if (pl) { r.pad1[0] = (uint8_t)m.proxy_port; r.pad1[1] = (uint8_t)(m.proxy_port >> 8); }
        if (st) { r.flags |= GM_REQ_INVALID; r.pad0[1] = (uint8_t)st; r.pad0[2] = (uint8_t)(st >> 8); }
        else {
            if ((flags >> 8) == 0) r.flags |= GM_REQ_HTTP10;
            if (flags & 2u) r.flags |= GM_REQ_CHUNKED;
        }
        for (int k = 0; k < 16; k++) r.rid[k] = m.rid[k];
        *rec = r;
    }
}

// ---- PROXY protocol intake (nginx 1.17.3 ngx_proxy_protocol_read, src/core/ngx_proxy_protocol.c):
// on a `listen ... proxy_protocol` port the connection starts with a v1 text or v2 binary header,
// read before the request.  k_wire_proxy (a lane per message, launched only when the generation
// has such a port) copies each descriptor, advances a header-bearing message past its header and
// puts the header's source address / port in the copy; a missing or broken header marks the copy
// WIRE_F_BROKEN (nginx closes the connection: status 444, no response).  WIRE_F_PADDR: the copy's
// paddr fields are the record's $proxy_protocol_addr / port (the parse passes copy them after raddr).
// ngx_atoi: decimal digits only, at least one, no overflow; -1 otherwise
__device__ __forceinline__ int64_t w_atoi(const uint8_t *p, uint32_t n) {
    if (n == 0) return -1;
    int64_t v = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!w_digit(p[i]) || v > (0x7FFFFFFFFFFFFFFFll - 9) / 10) return -1;
        v = v * 10 + (p[i] - '0');
    }
    return v;
}
// one header at b[0, n): the bytes it takes (ok), the source address text (plen 0: none) and port
__device__ uint32_t proxy_read(const uint8_t *b, uint32_t n, uint8_t *paddr, uint32_t &plen, uint32_t &pport,
                               bool &ok) {
    plen = 0; pport = 0; ok = false;
    static constexpr uint8_t SIG[12] = {'\r', '\n', '\r', '\n', 0, '\r', '\n', 'Q', 'U', 'I', 'T', '\n'};
    bool v2 = n >= 16;
    for (int k = 0; k < 12 && v2; k++) v2 = b[k] == SIG[k];
    if (v2) {   // ngx_proxy_protocol_v2_read
        if ((b[12] >> 4) != 2) return 0;                     // unknown version
        const uint32_t len = (uint32_t)b[14] << 8 | b[15];
        if (n - 16 < len) return 0;                          // header is too large
        const uint32_t end = 16 + len;
        ok = true;
        if ((b[12] & 15) != 1 || (b[13] & 15) != 1) return end;   // LOCAL / not STREAM: no address
        InetAddr a = {};
        const uint32_t fam = b[13] >> 4;
        if (fam == 1) {
            if (len < 12) { ok = false; return 0; }
            a.fam = 4;
            for (int k = 0; k < 4; k++) a.b[k] = b[16 + k];
            pport = (uint32_t)b[24] << 8 | b[25];
        } else if (fam == 2) {
            if (len < 36) { ok = false; return 0; }
            a.fam = 6;
            for (int k = 0; k < 16; k++) a.b[k] = b[16 + k];
            pport = (uint32_t)b[48] << 8 | b[49];
        } else {
            return end;                                      // AF_UNIX / unspecified: no address
        }
        plen = ngx_addr_text(a, paddr);
        return end;
    }
    if (n < 8 || b[0] != 'P' || b[1] != 'R' || b[2] != 'O' || b[3] != 'X' || b[4] != 'Y' || b[5] != ' ') return 0;
    uint32_t p = 6;
    if (n - 6 >= 7 && b[6] == 'U' && b[7] == 'N' && b[8] == 'K' && b[9] == 'N' && b[10] == 'O' && b[11] == 'W' &&
        b[12] == 'N') {
        p += 7;
    } else {
        if (n - 6 < 5 || b[6] != 'T' || b[7] != 'C' || b[8] != 'P' || (b[9] != '4' && b[9] != '6') || b[10] != ' ')
            return 0;
        p = 11;
        const uint32_t a0 = p;
        for (;;) {   // the source address: hex digits, ':' and '.', up to a space
            if (p == n) return 0;
            const uint32_t ch = b[p++];
            if (ch == ' ') break;
            if (ch != ':' && ch != '.' && w_hex(ch) < 0) return 0;
        }
        const uint32_t al = p - a0 - 1;
        for (;;) {   // the destination address
            if (p == n) return 0;
            if (b[p++] == ' ') break;
        }
        const uint32_t p0 = p;
        for (;;) {   // the source port, up to a space
            if (p == n) return 0;
            if (b[p++] == ' ') break;
        }
        const int64_t port = w_atoi(b + p0, p - p0 - 1);
        if (port < 0 || port > 65535) return 0;
        pport = (uint32_t)port;
        // (an address longer than any address text is kept as none: realip could not parse it)
        if (al <= PADDR_MAX) { for (uint32_t k = 0; k < al; k++) paddr[k] = b[a0 + k]; plen = al; }
    }
    for (; p + 1 < n; p++)   // the line's CRLF
        if (b[p] == '\r' && b[p + 1] == '\n') { ok = true; return p + 2; }
    plen = 0;
    return 0;
}
__global__ void k_wire_proxy(const uint8_t *__restrict__ W, const gm_wire_msg *__restrict__ in, uint32_t n, GTab t,
                             gm_wire_msg *__restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        gm_wire_msg m = in[i];
        bool proxy = false;
        for (uint32_t k = 0; k < t.n_ports; k++) proxy |= t.ports[k].port == m.port && t.ports[k].proxy;
        m.flags &= (uint8_t)~(WIRE_F_PADDR | WIRE_F_BROKEN);
        if (proxy && (m.flags & GM_WIRE_PROXY_DONE)) {   // a keep-alive request: the caller's copy
            if (m.paddr_len > PADDR_MAX) m.paddr_len = 0;
            m.flags |= WIRE_F_PADDR;
        } else if (proxy) {
            uint32_t plen, pport;
            bool ok;
            const uint32_t used = proxy_read(W + m.off, m.len, m.paddr, plen, pport, ok);
            m.paddr_len = (uint8_t)plen;
            m.proxy_port = (uint16_t)pport;
            // a header with no request after it: nginx waits for one, then times out and closes
            if (!ok || used >= m.len) { m.flags |= WIRE_F_BROKEN; m.paddr_len = 0; m.proxy_port = 0; }
            else { m.off += used; m.len -= used; m.flags |= WIRE_F_PADDR; }
        }
        out[i] = m;
    }
}

// The internal flags k_wire_proxy leaves in its copies (WIRE_F_*): every parse kernel takes them
// through fmask, which keeps them only when that pass ran -- on a generation without a
// proxy_protocol port the caller's own flag bits 0x20 / 0x80 mean nothing (ADVICE r5)
constexpr uint32_t WIRE_FMASK_PROXY = 0xFFu, WIRE_FMASK_PLAIN = 0xFFu & ~(uint32_t)(WIRE_F_PADDR | WIRE_F_BROKEN);

// A request pass 2 writes with the flat gather (k_wire_gather): an invalid one (kind 2: its
// record and address only), or a valid summary (kind 1) whose $uri is the path verbatim, with at
// most WIRE_PIECES chunks if its body came chunked.  The others (complex-URI paths, longer
// chunked bodies, re-parses) go to their wave's full list.  kf: kind | flags << 8, bit 31 = more
// chunks than recorded.
__device__ __forceinline__ bool wire_flat(uint32_t kf) {
    const uint32_t kind = kf & 0xFFu, flags = (kf >> 8) & 0xFFu;
    return kind == 2 || (kind == 1 && (flags & 1u) && !(kf >> 31));
}

// pass 1: slot size of every request (sizes[n] = 0 for the exclusive scan's total), and each
// wave's list of the requests pass 2 writes one at a time (full[gw * per + k], k < fcnt[gw]: the
// wave's own requests, so no atomic is taken; round 6)
__global__ __launch_bounds__(64 * WIRE_WAVES) WIRE_OCC void k_wire_size(const uint8_t *__restrict__ W,
                                                               const gm_wire_msg *__restrict__ msgs, uint32_t n,
                                                               uint64_t *__restrict__ sizes, uint8_t *__restrict__ gscr,
                                                               WireSum *__restrict__ sums, uint32_t fmask,
                                                               uint32_t *__restrict__ full, uint32_t per,
                                                               uint32_t *__restrict__ fcnt, uint2 *__restrict__ pieces) {
    __shared__ uint32_t tabs[WIRE_WAVES][WIRE_LINES];
    __shared__ uint4 stgs[WIRE_WAVES][WIRE_STAGE / 16];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t gw = blockIdx.x * WIRE_WAVES + wv;
    uint8_t *scr = gscr + ((uint64_t)blockIdx.x * WIRE_WAVES + wv) * WIRE_SCR;
    uint8_t *stg = reinterpret_cast<uint8_t *>(stgs[wv]);
    uint32_t nf = 0;
    for (uint32_t i = gw; i < n; i += gridDim.x * WIRE_WAVES) {
        const gm_wire_msg &m = msgs[i];
        uint32_t kf = 0;
        const uint64_t s = wire_one<false>(W, m, tabs[wv], scr, stg, lane, nullptr, 0, 0, nullptr, sums + i, fmask, &kf,
                                           pieces + (uint64_t)i * WIRE_PIECES);
        if (lane == 0) {
            sizes[i] = s;
            if (!wire_flat(kf)) full[(uint64_t)gw * per + nf++] = i;
        }
    }
    if (lane == 0) fcnt[gw] = nf;
    if (blockIdx.x == 0 && threadIdx.x == 0) sizes[n] = 0;
}

// pass 2a: the output block map -- blk[k] = the last request whose slot starts at or before byte
// k * 1024 (a lane per request: its slot covers blocks [ceil(base / 1K), ceil(next base / 1K)))
__global__ void k_wire_blk(const uint64_t *__restrict__ bases, uint32_t n, uint32_t *__restrict__ blk, uint32_t nblk) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        // (the last request's slot ends the arena: blocks up to its end, not the capacity's)
        const uint64_t k0 = i == 0 ? 0 : (bases[i] + 1023) >> 10, k1 = (bases[i + 1] + 1023) >> 10;
        for (uint64_t k = k0; k < k1 && k < nblk; k++) blk[k] = i;
    }
}

// a chunk of a flat slot: the segments of the request's record in field order -- $uri, $args, the
// header block, the body's pieces (WIRE_PIECES: its span, or a chunked body's chunks), host,
// method, $request_uri, raddr, paddr -- with q[k] = the segment's source address minus its slot
// offset (byte x of segment k is at q[k] + x) and their ends (every index below is a constant
// after unrolling: the struct stays in registers)
constexpr int WIRE_FSEGS = 8 + WIRE_PIECES;
struct WireFlat {
    uint64_t q[WIRE_FSEGS];
    uint32_t end[WIRE_FSEGS];
};
__device__ __forceinline__ void flat_seg(const WireFlat &g, uint32_t s, uint64_t &q, uint32_t &st, uint32_t &e) {
    q = g.q[WIRE_FSEGS - 1]; e = g.end[WIRE_FSEGS - 1]; st = g.end[WIRE_FSEGS - 2];
#pragma unroll
    for (int k = WIRE_FSEGS - 2; k >= 0; k--)
        if (s == (uint32_t)k) { q = g.q[k]; e = g.end[k]; st = k ? g.end[k > 0 ? k - 1 : 0] : 0u; }
}
// the 16 bytes at slot offset o: five funnel-shifted dwords when they lie in one segment, else the
// bytes one by one (the segment advanced as they cross its end); zero past the total
__device__ __forceinline__ uint4 wire_flat_chunk(const WireFlat &g, uint32_t o) {
    const uint32_t total = g.end[WIRE_FSEGS - 1];
    if (o >= total) return make_uint4(0, 0, 0, 0);
    uint32_t sg = 0;
#pragma unroll
    for (int k = 0; k < WIRE_FSEGS - 1; k++) sg += o >= g.end[k] ? 1u : 0u;
    uint64_t q; uint32_t st, en;
    flat_seg(g, sg, q, st, en);
    const uint64_t src = q + o;
    const uint32_t sh = (uint32_t)(src & 3);
    if (o + 16 <= en && (o - st) + 20 <= (en - st) + sh) {
        const uint32_t *a = reinterpret_cast<const uint32_t *>(src - sh);
        uint32_t d[5];
#pragma unroll
        for (int k = 0; k < 5; k++) d[k] = a[k];
        return make_uint4(__builtin_amdgcn_alignbyte(d[1], d[0], sh), __builtin_amdgcn_alignbyte(d[2], d[1], sh),
                          __builtin_amdgcn_alignbyte(d[3], d[2], sh), __builtin_amdgcn_alignbyte(d[4], d[3], sh));
    }
    uint32_t w[4] = {0, 0, 0, 0};
    uint32_t s2 = sg;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t oj = o + j;
        while (oj >= en && s2 < WIRE_FSEGS - 1) { s2++; flat_seg(g, s2, q, st, en); }   // (segments may be empty)
        const uint32_t x = oj < total ? (uint32_t)*reinterpret_cast<const uint8_t *>(q + oj) : 0u;
        w[j >> 2] |= x << (8 * (j & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// pass 2b: the flat requests' slots, a lane per 16-byte output chunk over the whole arena (every
// load of a wave's 64 chunks in flight together; round 6: one wave per request writing its fields
// one after another ran 7.9 ms per 2M messages), and each one's record by the lane of its first
// chunk.  The arena length and the capacity check too.
__global__ __launch_bounds__(256) void k_wire_gather(const uint8_t *__restrict__ W, const gm_wire_msg *__restrict__ msgs,
                                                     uint32_t n, const uint64_t *__restrict__ sizes,
                                                     const uint64_t *__restrict__ bases, gm_req *__restrict__ reqs,
                                                     uint8_t *__restrict__ out, uint64_t cap,
                                                     uint64_t *__restrict__ arena_len, uint32_t *__restrict__ status,
                                                     const WireSum *__restrict__ sums, const uint32_t *__restrict__ blk,
                                                     uint32_t fmask, const uint2 *__restrict__ pieces) {
    const uint64_t total = bases[n];
    const uint64_t capa = cap & ~15ull;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *arena_len = min(total, capa);
        if (total > capa) atomicOr(status + 3, 32u);
    }
    const uint64_t end = min(total, capa);
    for (uint64_t o = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) * 16; o < end; o += (uint64_t)gridDim.x * blockDim.x * 16) {
        uint32_t i = blk[o >> 10];
        while (i + 1 < n && bases[i + 1] <= o) i++;
        const uint64_t base = bases[i], slot = sizes[i];
        if (base + slot > capa || o >= base + slot) continue;   // (void: k_wire_void writes its record)
        const WireSum &sm = sums[i];
        const uint32_t kind = sm.kind, flags = sm.flags, np = sm.pad0;
        if (!wire_flat(kind | flags << 8 | ((flags & 2u) && np > WIRE_PIECES ? 1u << 31 : 0u))) continue;   // the full list's
        const gm_wire_msg &m = msgs[i];
        const uint8_t *b = W + m.off;
        const uint32_t ra = min((uint32_t)m.raddr_len, 40u);
        const uint32_t pa = ((m.flags & fmask) & WIRE_F_PADDR) ? min((uint32_t)m.paddr_len, PADDR_MAX) : 0u;
        const bool ok = kind == 1;   // (kind 2: the record and the addresses only)
        const uint32_t path_off = sm.path_off, target_off = sm.target_off;
        uint32_t len[WIRE_FSEGS];
        const uint8_t *ptr[WIRE_FSEGS];
        len[0] = ok ? sm.uri_len : 0u; len[1] = ok ? sm.args_len : 0u; len[2] = ok ? sm.hdrs_len : 0u;
        ptr[0] = path_off == GM_NONE ? reinterpret_cast<const uint8_t *>(WIRE_SLASH) : b + path_off;
        ptr[1] = b + sm.args_off; ptr[2] = b + sm.hdr_off;
        if (ok && (flags & 2u)) {   // a chunked body: its recorded chunks
            const uint4 *pp = reinterpret_cast<const uint4 *>(pieces + (uint64_t)i * WIRE_PIECES);
#pragma unroll
            for (int k = 0; k < WIRE_PIECES / 2; k++) {
                const uint4 v = pp[k];
                const bool a0 = 2u * k < np, a1 = 2u * k + 1 < np;
                ptr[3 + 2 * k] = b + (a0 ? v.x : 0u); len[3 + 2 * k] = a0 ? v.y : 0u;
                ptr[4 + 2 * k] = b + (a1 ? v.z : 0u); len[4 + 2 * k] = a1 ? v.w : 0u;
            }
        } else {
            ptr[3] = b + sm.body0; len[3] = ok ? sm.body_len : 0u;
#pragma unroll
            for (int k = 1; k < WIRE_PIECES; k++) { ptr[3 + k] = b; len[3 + k] = 0; }
        }
        ptr[3 + WIRE_PIECES] = b + sm.host_off; len[3 + WIRE_PIECES] = ok ? sm.host_len : 0u;
        ptr[4 + WIRE_PIECES] = b + sm.method_off; len[4 + WIRE_PIECES] = ok ? sm.method_len : 0u;
        ptr[5 + WIRE_PIECES] = target_off == GM_NONE ? reinterpret_cast<const uint8_t *>(WIRE_SLASH) : b + target_off;
        len[5 + WIRE_PIECES] = ok ? sm.target_len : 0u;
        ptr[6 + WIRE_PIECES] = m.raddr; len[6 + WIRE_PIECES] = ra;
        ptr[7 + WIRE_PIECES] = m.paddr; len[7 + WIRE_PIECES] = pa;
        WireFlat g;
        uint32_t e = 0;
#pragma unroll
        for (int k = 0; k < WIRE_FSEGS; k++) {
            g.q[k] = reinterpret_cast<uint64_t>(ptr[k]) - e;
            e += len[k];
            g.end[k] = e;
        }
        const uint32_t rel = (uint32_t)(o - base);
        *reinterpret_cast<uint4 *>(out + o) = wire_flat_chunk(g, rel);
        if (rel == 0) {
            gm_req r = {};
            r.base = base;
            if (ok) {
                r.uri_len = sm.uri_len; r.args_len = sm.args_len; r.hdr_len = sm.hdrs_len; r.body_len = sm.body_len;
                r.host_len = (uint16_t)sm.host_len; r.method_len = (uint16_t)sm.method_len;
                r.ruri_len = (uint16_t)sm.target_len;
            }
            r.raddr_len = (uint16_t)ra;
            r.port = m.port; r.remote_port = m.remote_port;
            r.flags = m.flags & (GM_REQ_HTTPS | GM_REQ_HTTP2);
            r.pad0[0] = (uint8_t)pa;
            if (pa) { r.pad1[0] = (uint8_t)m.proxy_port; r.pad1[1] = (uint8_t)(m.proxy_port >> 8); }
            if (!ok) {
                const uint32_t st = sm.status;
                r.flags |= GM_REQ_INVALID; r.pad0[1] = (uint8_t)st; r.pad0[2] = (uint8_t)(st >> 8);
            } else {
                if ((flags >> 8) == 0) r.flags |= GM_REQ_HTTP10;
                if (flags & 2u) r.flags |= GM_REQ_CHUNKED;
            }
            for (int k = 0; k < 16; k++) r.rid[k] = m.rid[k];
            reqs[i] = r;
        }
    }
}

// pass 2c: the records no slot byte carries, a lane per request.  A zero-size slot inside the
// capacity (an invalid request -- kind 2 -- without a connection address or a PROXY address: no
// output chunk is its first, so k_wire_gather never reaches it) gets its empty record with pass
// 1's status.  In a void batch (the arena capacity exceeded: gm_sync reports GM_E_OVERFLOW) every
// request whose slot lies past the capacity gets an empty invalid record (500) inside it, so the
// layout stays legal.
__global__ void k_wire_void(const gm_wire_msg *__restrict__ msgs, uint32_t n, const uint64_t *__restrict__ sizes,
                            const uint64_t *__restrict__ bases, gm_req *__restrict__ reqs, uint64_t cap,
                            const WireSum *__restrict__ sums) {
    const uint64_t capa = cap & ~15ull;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint64_t base = bases[i], slot = sizes[i];
        const bool fits = base + slot <= capa;
        if (fits && slot != 0) continue;
        const gm_wire_msg &m = msgs[i];
        const uint32_t st = fits ? sums[i].status : 500u;
        gm_req r = {};
        r.base = min(base, capa);
        r.port = m.port; r.remote_port = m.remote_port;
        r.flags = (m.flags & (GM_REQ_HTTPS | GM_REQ_HTTP2)) | GM_REQ_INVALID;
        r.pad0[1] = (uint8_t)st; r.pad0[2] = (uint8_t)(st >> 8);
        for (int k = 0; k < 16; k++) r.rid[k] = m.rid[k];
        reqs[i] = r;
    }
}

// pass 2d: the full lists -- each wave its own requests from pass 1 (complex-URI paths, chunked
// bodies, invalid requests, re-parses), one request at a time
__global__ __launch_bounds__(64 * WIRE_WAVES) WIRE_OCC_EMIT void k_wire_emit_full(const uint8_t *__restrict__ W,
                                                               const gm_wire_msg *__restrict__ msgs, uint32_t n,
                                                               const uint64_t *__restrict__ sizes,
                                                               const uint64_t *__restrict__ bases,
                                                               gm_req *__restrict__ reqs, uint8_t *__restrict__ out,
                                                               uint64_t cap, uint8_t *__restrict__ gscr,
                                                               const WireSum *__restrict__ sums, uint32_t fmask,
                                                               const uint32_t *__restrict__ full, uint32_t per,
                                                               const uint32_t *__restrict__ fcnt) {
    __shared__ uint32_t tabs[WIRE_WAVES][WIRE_LINES];
    __shared__ uint4 stgs[WIRE_WAVES][WIRE_STAGE / 16];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t gw = blockIdx.x * WIRE_WAVES + wv;
    uint8_t *scr = gscr + ((uint64_t)blockIdx.x * WIRE_WAVES + wv) * WIRE_SCR;
    uint8_t *stg = reinterpret_cast<uint8_t *>(stgs[wv]);
    const uint64_t capa = cap & ~15ull;
    const uint32_t nf = __builtin_amdgcn_readfirstlane(fcnt[gw]);
    for (uint32_t k = 0; k < nf; k++) {
        const uint32_t i = __builtin_amdgcn_readfirstlane(full[(uint64_t)gw * per + k]);
        const uint64_t base = bases[i], slot = sizes[i];
        if (base + slot > capa) continue;   // (void: k_wire_void)
        const uint32_t kind = wv_bcast(sums[i].kind);
        if (kind != 0) wire_emit_sum<false>(W, msgs[i], sums[i], scr, lane, out, base, slot, reqs + i, fmask);
        else wire_one<true>(W, msgs[i], tabs[wv], scr, stg, lane, out, base, slot, reqs + i, nullptr, fmask);
    }
}
