// gm_ws.inc -- the WebSocket frame parser (`wallarm_parse_websocket`), included into gm_device.hip's
// anonymous namespace: the unmasked message view V of a segment of client-to-server bytes, one wave
// (64 lanes) per segment.
//
// THE GRAMMAR (include/gpumatch.h states the same; tests/ws_reference.py restates it in Python).
// A segment is a run of one connection's client-to-server bytes.  It begins at a frame boundary with
// no message open.  Frames (RFC 6455) are read left to right.
// Header.  Byte 0 is FIN | RSV1-3 | opcode, byte 1 is MASK | len7.  len7 == 126 is followed by a
//   16-bit, len7 == 127 by a 64-bit big-endian length.  The 4-byte masking key follows the length.
//   Payload byte k is wire ^ key[k & 3].
// Protocol errors stop the segment with GM_WS_PROTO and a reason.  The first two bytes are judged as
//   soon as both are there, and the first reason that applies, in this order, is reported:
//   RSV        RSV2 or RSV3 set, or RSV1 set on a control or continuation frame
//   OPCODE     opcode 3-7 or 0xB-0xF
//   UNMASKED   MASK = 0
//   CTRL_FRAG  a control frame with FIN = 0
//   CTRL_LEN   a control frame with len7 > 125
//   CONT       opcode 0 with no message open
//   NESTED     opcode 1 or 2 while a message is open
//   LENGTH     (once the length's bytes are there) a 16-bit form holding a value < 126, a 64-bit form
//              holding a value < 65536, or the 64-bit form's top bit set
// Compression.  RSV1 on an opcode-1 or opcode-2 frame that passes the checks above (permessage-
//   deflate) stops before that frame with GM_WS_DEFLATE: it is not inflated.
// Incomplete frame.  A frame whose header or payload runs past the segment's end stops with GM_WS_OK.
// Close.  A complete close frame (opcode 8) stops with GM_WS_CLOSED, consumed = the offset after it.
// Ping and pong payloads are not emitted.
// The view V.  For every complete data message in order -- an opcode-1 or -2 frame, then continuation
//   frames, up to FIN = 1, control frames allowed in between -- its fragments' unmasked payloads
//   joined, then '\n'.  No UTF-8 validation.  out_len covers complete messages only: a message still
//   open at the stop contributes nothing (its bytes may lie in the slot past out_len); n_messages
//   counts the complete ones.
// Offsets.  stop = the offset of the frame at which reading stopped (len: the segment was read out).
//   consumed = the offset after the last frame behind which no message was open: the caller submits
//   the connection's bytes from there again, with what arrived since.
//
// SIZE BOUND: |V| <= len, so segment i's slot is len bytes.  A payload byte maps 1 -> 1; a message's
// '\n' is charged to a header byte of its last frame, and every frame has at least 6.
//
// WORK SPLIT.  k_ws_size (a lane per segment) gives the slot sizes, one exclusive scan the slots;
// k_ws's persistent workgroups pull segments from a queue, a wave owning a segment, <= 1 KiB a step:
// (1) Load: a step's window starts at any byte w0 (the next header, or where the last window ended
//     inside a payload).  Lane l loads the 16-byte granule l from the granule that holds w0, through
//     a buffer resource that ends with the segment's last granule (a read past it returns 0), into
//     the wave's LDS input row; lane 0 adds the granule after the window, so a header that begins in
//     the window is whole in the row.
// (2) Walk: frame boundaries are a dependent chain, so the wave walks them in uniform control flow:
//     the header at p is read from the row at a wave-uniform address (five aligned dwords, funnel-
//     shifted), validated, and a data frame is appended to the LDS frame table as
//     {payload start, payload end, key, flags} in ROW coordinates, clipped to the window, the key
//     already rotated to the row's dword phase (a lane's dwords all lie at row offsets = 0 mod 4, so
//     one rotation per frame and step serves every lane).  On the way each lane counts the entries
//     that end before its granule: its first entry.  The walk stops at the window's end or
//     when the table is full; the step ends there, and the next one starts at the next header, not
//     at a fixed stride.  A payload that runs past the step is carried state (its start, end, key
//     and flags: the next step's entry 0), beside the message-open bit, the output cursor and the
//     committed length; a header that began in the window needs no second read.
// (3) Unmask: a lane runs over the entries that meet its 16 bytes (several tiny frames may), XORs its
//     dwords with the entry's key under the byte mask of the payload's part, and builds the emit
//     mask.  A message's '\n' goes where its last fragment's payload ends: in place of the next
//     frame's first header byte, or, behind the last frame of a step, as the carried entry's.
// (4) Compaction: popcount, wave prefix sum, the bytes into the LDS output row; whole 16-byte vectors
//     leave as aligned vector stores, the slot's ragged ends byte by byte, the tail below 16 bytes
//     is carried (xml_flush).  out_len is the cursor at the last commit.  Every write is a vector store.

constexpr uint32_t WS_BLOCK = 256, WS_WAVES = WS_BLOCK / 64;
constexpr uint32_t WS_STEP = 1024;
constexpr uint32_t WS_TAB = 64;                              // frame table entries of one step
constexpr uint32_t WS_STATUS_WORD = UPURI_STATUS_WORD + 4;   // gm_ws_messages: output capacity exceeded
constexpr uint32_t WS_EMIT = 1u, WS_NL = 2u;                 // entry flags: (always) a data payload; '\n' at its end

struct WsLds {            // one wave's
    XmlLds io;            // in: the window's granules + the one after; out: the carried tail, the step's output
    uint4 tab[WS_TAB];    // {payload start, payload end, rotated key, flags}, row coordinates
};
struct WsShared { WsLds w[WS_WAVES]; };
static_assert(sizeof(WsShared) <= 20 * 1024, "the xml kernel's LDS budget: 8 workgroups per CU");
static_assert(sizeof(gm_ws_seg) == 16 && sizeof(gm_ws_result) == 16, "gpumatch.h");

// a frame [ps, pe) of the segment with its key, as an entry of the step whose row byte `sk` is
// segment byte w0 and whose window ends at wend (pe > wend: clipped, and its '\n' is a later step's)
__device__ __forceinline__ uint4 ws_entry(uint32_t ps, uint32_t pe, uint32_t key, uint32_t flags, uint32_t w0, uint32_t sk,
                                          uint32_t wend) {
    const uint32_t rs = max(ps, w0) - w0 + sk, re = min(pe, wend) - w0 + sk;
    // row byte r is payload byte w0 - sk + r - ps: a row dword's byte b takes key[(w0 - sk - ps + b) & 3]
    return make_uint4(rs, re, __builtin_rotateright32(key, 8 * ((w0 - sk - ps) & 3)), pe > wend ? flags & ~WS_NL : flags);
}

__device__ __forceinline__ uint32_t ws_bytes(uint32_t nib) {   // a nibble's bits as a dword's byte masks
    return (nib & 1 ? 0xFFu : 0u) | (nib & 2 ? 0xFF00u : 0u) | (nib & 4 ? 0xFF0000u : 0u) | (nib & 8 ? 0xFF000000u : 0u);
}

// The view of the segment src[0, n) -> dst[0, <= n): the result, and the view's length in vlen.
__device__ gm_ws_result ws_segment(WsLds &W, const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t lane, uint32_t &vlen) {
    XmlOut O;
    O.dmis = (uint32_t)((uintptr_t)dst & 15);
    O.base = dst - O.dmis;
    O.gpos = 0;
    O.T = O.dmis;
    O.limit = O.dmis + n;
    // the walk's state, wave-uniform: p = the next header; cps .. cfl = the carried frame
    uint32_t p = 0, w0 = 0, consumed = 0, nmsg = 0, ocur = 0, committed = 0, status = GM_WS_OK;
    uint32_t cps = 0, cpe = 0, ckey = 0, cfl = 0;
    bool open = false, stopped = n == 0;
    const uint32_t l0 = 16 * lane;
    while (!stopped) {
        // ---- (1) load: row byte sk = segment byte w0; the resource ends with the segment's last granule
        const uint32_t sk = (uint32_t)((uintptr_t)(src + w0) & 15);
        const uint32_t wend = w0 + min(n - w0, WS_STEP - sk);
        const uint32_t nrec = (uint32_t)min((uint64_t)WS_STEP + 16, ((uint64_t)sk + (n - w0) + 15) & ~15ull);
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(src + w0 - sk), (short)0, (int)nrec, 0x00020000);
        uint32_t w[4], x[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) w[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(l0 + 4 * j), 0, 0);
        if (lane == 0) {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) x[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(WS_STEP + 4 * j), 0, 0);
        }
        *reinterpret_cast<uint4 *>(W.io.in + l0) = make_uint4(w[0], w[1], w[2], w[3]);
        if (lane == 0) *reinterpret_cast<uint4 *>(W.io.in + WS_STEP) = make_uint4(x[0], x[1], x[2], x[3]);
        infl_sync();
        // ---- (2) the walk, in uniform control flow; `first` = the lane's count of entries that end before its bytes
        uint32_t nt = 0, first = 0;
        if (cfl) {
            const uint4 e = ws_entry(cps, cpe, ckey, cfl, w0, sk, wend);
            if (lane == 0) W.tab[0] = e;
            first += e.y < l0 ? 1u : 0u;
            nt = 1;
        }
        const uint32_t *row32 = reinterpret_cast<const uint32_t *>(W.io.in);
        for (;;) {
            if (p >= wend || nt == WS_TAB) break;   // (p <= n, wend <= n: p == n ends the walk here)
            // the 16 bytes from p: five aligned dwords of the row, shifted (p < wend: inside the row)
            const uint32_t rp = p - w0 + sk, q = rp >> 2, sh = 8 * (rp & 3);
            const uint32_t d0 = infl_u(row32[q]), d1 = infl_u(row32[q + 1]), d2 = infl_u(row32[q + 2]),
                           d3 = infl_u(row32[q + 3]), d4 = infl_u(row32[q + 4]);
            const uint64_t lo = (uint64_t)__builtin_amdgcn_alignbit(d1, d0, sh) | (uint64_t)__builtin_amdgcn_alignbit(d2, d1, sh) << 32;
            const uint64_t hi = (uint64_t)__builtin_amdgcn_alignbit(d3, d2, sh) | (uint64_t)__builtin_amdgcn_alignbit(d4, d3, sh) << 32;
            const uint32_t avail = n - p;
            stopped = true;   // (every way out of this frame but its end stops the segment)
            if (avail < 2) break;
            const uint32_t b0 = (uint32_t)lo & 0xFFu, b1 = (uint32_t)(lo >> 8) & 0xFFu;
            const uint32_t op = b0 & 15u, len7 = b1 & 127u;
            const bool fin = b0 & 0x80u, rsv1 = b0 & 0x40u, ctrl = op & 8u;
            uint32_t reason = 0;
            if ((b0 & 0x30u) || (rsv1 && (ctrl || op == 0))) reason = GM_WS_R_RSV;
            else if ((op >= 3 && op <= 7) || op >= 0xB) reason = GM_WS_R_OPCODE;
            else if (!(b1 & 0x80u)) reason = GM_WS_R_UNMASKED;
            else if (ctrl && !fin) reason = GM_WS_R_CTRL_FRAG;
            else if (ctrl && len7 > 125) reason = GM_WS_R_CTRL_LEN;
            else if (op == 0 && !open) reason = GM_WS_R_CONT;
            else if ((op == 1 || op == 2) && open) reason = GM_WS_R_NESTED;
            if (reason) { status = GM_WS_PROTO | reason << 8; break; }
            if (rsv1) { status = GM_WS_DEFLATE; break; }
            const uint32_t ext = len7 == 126 ? 2u : len7 == 127 ? 8u : 0u, hl = 2 + ext + 4;
            if (avail < 2 + ext) break;
            uint64_t plen = len7;
            uint32_t key = (uint32_t)(lo >> 16);
            if (ext == 2) {
                plen = ((uint32_t)(lo >> 16) & 0xFFu) << 8 | ((uint32_t)(lo >> 24) & 0xFFu);
                key = (uint32_t)(lo >> 32);
                if (plen < 126) { status = GM_WS_PROTO | GM_WS_R_LENGTH << 8; break; }
            } else if (ext == 8) {
                plen = __builtin_bswap64(lo >> 16 | hi << 48);
                key = (uint32_t)(hi >> 16);
                if (plen < 65536 || plen >> 63) { status = GM_WS_PROTO | GM_WS_R_LENGTH << 8; break; }
            }
            if (avail < hl || plen > avail - hl) break;   // the frame runs past the segment
            const uint32_t ps = p + hl, pe = ps + (uint32_t)plen;
            if (op == 8) { status = GM_WS_CLOSED; consumed = pe; break; }
            stopped = false;
            if (!ctrl) {
                const uint32_t fl = WS_EMIT | (fin ? WS_NL : 0u);
                const uint4 e = ws_entry(ps, pe, key, fl, w0, sk, wend);
                if (lane == 0) W.tab[nt] = e;
                first += e.y < l0 ? 1u : 0u;
                nt++;
                cps = ps; cpe = pe; ckey = key; cfl = fl;
                ocur += (uint32_t)plen;
                open = !fin;
                if (fin) { ocur++; committed = ocur; nmsg++; }
            }
            p = pe;
            if (!open) consumed = p;
        }
        // the step ends at the next header (or the stop), or the window's end; the last entry is
        // carried if its payload, or its '\n', lies there or behind
        const uint32_t send = min(p, wend);
        if (!(cfl && (cpe > send || (cpe == send && (cfl & WS_NL))))) cfl = 0;
        if (p == n && !(cfl && cpe > send)) stopped = true;   // read out, and no payload left behind the step
        infl_sync();
        // ---- (3) unmask: the entries that meet the lane's bytes [l0, l0 + 16) of the row
        uint32_t emask = 0;
        for (uint32_t k = first; k < nt; k++) {
            const uint4 e = W.tab[k];
            if (e.x >= l0 + 16) break;
            const uint32_t a = max(e.x, l0) - l0, b = min(e.y, l0 + 16) - l0;   // (e.y >= l0: by `first`)
            if (b > a) {
                const uint32_t m = ((1u << b) - 1) & ~((1u << a) - 1);
                emask |= m;
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) w[j] ^= e.z & ws_bytes((m >> (4 * j)) & 15u);
            }
            const uint32_t nl = e.y - l0;
            if ((e.w & WS_NL) && nl < 16) {
                emask |= 1u << nl;
                const uint32_t s8 = 8 * (nl & 3);
#pragma unroll
                for (uint32_t j = 0; j < 4; j++)
                    if ((nl >> 2) == j) w[j] = (w[j] & ~(0xFFu << s8)) | (uint32_t)'\n' << s8;
            }
        }
        // only the step's bytes: row [sk, send - w0 + sk)
        const uint32_t sendr = send - w0 + sk;
        const uint32_t vlo = sk > l0 ? min(sk - l0, 16u) : 0u, vhi = sendr > l0 ? min(sendr - l0, 16u) : 0u;
        emask &= ((1u << vhi) - 1) & ~((1u << vlo) - 1);
        // ---- (4) compaction into the output row, whole vectors out
        const uint32_t cnt = (uint32_t)__popc(emask);
        uint32_t pre = cnt;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(pre, d);
            if (lane >= d) pre += t;
        }
        const uint32_t sum = (uint32_t)__builtin_amdgcn_readlane((int)pre, 63);
        uint32_t pos = O.T + pre - cnt;
        if (emask == 0xFFFFu) {   // (inside a payload: the sixteen bytes)
#pragma unroll
            for (uint32_t j = 0; j < 16; j++) W.io.out[pos + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 16; j++)
                if (emask >> j & 1) W.io.out[pos++] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        }
        O.T += sum;
        infl_sync();   // (also: the row's and the table's reads above before the next step's writes)
        xml_flush(W.io, O, lane, false);
        w0 = cfl ? send : p;   // (no carry: p may lie past the window, behind a ping's payload)
    }
    // the '\n' of a message whose last payload byte was the last byte read
    if (cfl) {
        if (lane == 0) W.io.out[O.T] = '\n';
        O.T++;
    }
    infl_sync();
    xml_flush(W.io, O, lane, true);
    vlen = committed;
    gm_ws_result r;
    r.status = status; r.consumed = consumed; r.stop = p; r.n_messages = nmsg;
    return r;
}

// lim[i] = the slot of segment i (its len); k_ws's queue head (ctl[0]) reset
__global__ void k_ws_size(const gm_ws_seg *__restrict__ segs, uint32_t n, uint64_t *__restrict__ lim, uint32_t *__restrict__ ctl) {
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl[0] = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        lim[i] = segs[i].len;
        if (i + 1 == n) lim[n] = 0;
    }
}

// persistent workgroups: each wave pulls the next segment and writes its view to out[off[i] ...)
__global__ __launch_bounds__(WS_BLOCK) void k_ws(const uint8_t *__restrict__ wire, const gm_ws_seg *__restrict__ segs, uint32_t n,
                                                 uint32_t *__restrict__ ctl, uint8_t *__restrict__ out, uint64_t out_cap,
                                                 const uint64_t *__restrict__ off, uint32_t *__restrict__ len_out,
                                                 gm_ws_result *__restrict__ res, uint32_t *__restrict__ ov) {
    __shared__ WsShared sh;
    WsLds &W = sh.w[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63;
    // As in k_xml: one back edge, no lane-divergent branch at the loop's level.
    for (;;) {
        const uint32_t i = infl_u(atomicAdd(ctl, lane == 0 ? 1u : 0u));   // (lane 0: the value before the wave's add)
        if (i >= n) break;
        const uint8_t *src = wire + uniform64(segs[i].off);
        const uint32_t slen = infl_u(segs[i].len);
        const uint64_t o = uniform64(off[i]);
        const bool fits = o + slen <= out_cap;
        gm_ws_result r;
        r.status = GM_WS_OK; r.consumed = 0; r.stop = 0; r.n_messages = 0;
        uint32_t vlen = GM_NONE;
        if (fits) r = ws_segment(W, src, slen, out + o, lane, vlen);
        len_out[i] = infl_u(vlen);   // (the same words from every lane: one store each)
        *reinterpret_cast<uint4 *>(res + i) = make_uint4(infl_u(r.status), infl_u(r.consumed), infl_u(r.stop), infl_u(r.n_messages));
        atomicOr(ov, lane == 0 && !fits ? 1u : 0u);
    }
}
