// gm_xml.inc -- the xml request parser (SURVEY.md §8 f4, Wallarm's `xml` parser), included into
// gm_device.hip's anonymous namespace: the character-data view X of an XML body, one wave (64
// lanes) per body.
//
// THE GRAMMAR (include/gpumatch.h states the same; tests/xml_reference.py restates it in Python).
// It is lenient on purpose: a WAF view, not a well-formedness check.
// Which bodies.  body_len > 0 and one of: the value of the request's first Content-Type header (the
//   one body_kind reads) contains "xml", ASCII case-insensitively; or the body, after an optional
//   EF BB BF and any run of space, tab, CR and LF, begins with "<?xml" (case-sensitive).  The body
//   is read as sent: it is not inflated first, and a multipart part is not read as XML.
// Scan.  Left to right from offset 0, starting in text.  At position p in text:
//   "<!--"       a comment: it ends after the first "-->" that starts at q >= p + 2 (so "<!-->" is
//                a whole comment).  Nothing is emitted: the text on either side joins.
//   "<![CDATA["  the bytes up to the first "]]>" at q >= p + 9 are emitted verbatim (no reference
//                decoding); the scan continues at q + 3.  A later "<![CDATA[" inside is content.
//   "<?"         ends after the first "?>" at q >= p + 1 (so "<?>" is whole).  Nothing is emitted.
//   "<!" else    a declaration: '[' enters the subset, ']' leaves it, the first '>' outside the
//                subset ends it.  Quotes are not considered.  Nothing is emitted.
//   '<' else     a tag: '\n' is emitted for the '<'.  Outside quotes '"' or ''' opens a quoted string
//                that runs to the next same quote; its bytes are character data and its closing
//                quote emits '\n'.  '>' outside quotes ends the tag.  Every other tag byte is dropped.
//   other bytes  character data.
//   A construct that the body's end cuts short just ends: what it emitted so far stands.
// Character data (text and quoted strings) is emitted as is, except references.  At '&' one of
//   "&lt;" "&gt;" "&amp;" "&quot;" "&apos;" (case-sensitive), "&#" [0-9]{1,8} ";",
//   "&#x" or "&#X" [0-9A-Fa-f]{1,8} ";" is replaced by the byte or by the UTF-8 of v, where
//   1 <= v <= 0x10FFFF outside D800-DFFF.  Anything else leaves the '&' an ordinary byte.  The
//   output is not decoded again: "&amp;lt;" gives "&lt;".
// Out of scope: entity declarations of a DOCTYPE are not expanded; tag and attribute names are not
//   emitted; unquoted attribute values are not emitted; encodings that are not ASCII-compatible are
//   not handled; quotes inside declarations are not considered.
//
// SIZE BOUND: |X| <= body_len, so request i's slot is body_len bytes.  Every output byte is charged
// to an input byte of its own: text and CDATA 1 -> 1; a tag's '<' and a closing quote 1 -> 1 (the
// '\n'); a reference of n >= 4 input bytes yields <= 4 output bytes and <= n in every case ("&#128;"
// 6 -> 2, "&#2048;" 7 -> 3, "&#65536;" 8 -> 4: a value that needs k UTF-8 bytes needs >= k - 1 + 2
// digits in decimal and >= k digits in hex, behind "&#" and before ';').  Input bytes are disjoint.
//
// WORK SPLIT.  k_xml_size (a lane per request) applies the selection rule and lists the XML bodies;
// k_xml's persistent workgroups pull from the list, a wave owning a body, 1 KiB a step:
// (1) Load: lane l loads 16 bytes through a buffer resource over the body's 16-byte granules (a read
//     past it returns 0), zeroes what lies outside the body and puts them into the wave's LDS input
//     row; the row keeps the step's last 16 bytes in front and lane 0 adds the 16 bytes after the
//     step, so a lane reads its neighbours (up to 8 bytes back, 8 ahead) from the row.
// (2) Classes: the event bytes ('<' '>' '"' ''' '[' ']') are found by a SWAR compare of the lane's four
//     dwords; each gets an event class from a local pattern ('<' by what follows, '>' by what
//     precedes, the '[' that ends "<![CDATA[", the others by themselves); every other byte: none.
// (3) The state scan: a class is a map state -> state over ten states, 4-bit fields of a 64-bit word.
//     A lane composes the maps of its event bytes, an inclusive wave scan (__shfl_up, six rounds)
//     composes the lanes' maps, and the step's carried-in state through lane l - 1's prefix is lane
//     l's start state; lane 63's end state is carried.  A step costs the same however many tags.
// (4) Emit: the lane replays its events from its start state (the state holds over the bytes between
//     two events, so a run is kept or dropped as one mask) into an emit mask and output bytes.
//     A reference holds no event byte, so "byte x lies in a valid reference" is a property of the raw
//     bytes: each '&' in [x0 - 11, x0 + 16) is parsed from the LDS row, its <= 4 output bytes go to its
//     first input positions, and it counts if the state there is character data.
// (5) Compaction: popcount per lane, wave prefix sum, the bytes into the wave's LDS output row; the
//     row's whole 16-byte vectors leave as aligned 16-byte stores (the slot's first and last partial
//     vector byte by byte), the tail below 16 bytes is carried.  Every write to memory is a vector store.

constexpr uint32_t XML_BLOCK = 256, XML_WAVES = XML_BLOCK / 64;
constexpr uint32_t XML_STEP = 1024;
// control words of one launch: [0] bodies listed, [1] the list's queue head, [2] views given, [3] overflow
constexpr uint32_t XML_CTL_WORDS = 4;
constexpr uint32_t XML_VIEWS_WORD = 26;                      // batch status word: bodies given a view
constexpr uint32_t XML_STATUS_WORD = UPURI_STATUS_WORD + 3;  // gm_xml_bodies: output capacity exceeded

enum : uint32_t { XS_TEXT, XS_TAG, XS_DQ, XS_SQ, XS_COMMENT, XS_COPEN, XS_CDATA, XS_PI, XS_DECL, XS_SUBSET, XS_N };
enum : uint32_t { XC_NONE, XC_LT_TAG, XC_LT_COMMENT, XC_LT_CDATA, XC_LT_PI, XC_LT_DECL, XC_GT, XC_GT_DASH, XC_GT_BRK,
                  XC_GT_Q, XC_DQ, XC_SQ, XC_LB, XC_LB_CDATA, XC_RB, XC_N };

constexpr uint32_t xml_step(uint32_t s, uint32_t c) {
    switch (c) {
    case XC_LT_TAG: return s == XS_TEXT ? XS_TAG : s;
    case XC_LT_COMMENT: return s == XS_TEXT ? XS_COMMENT : s;
    case XC_LT_CDATA: return s == XS_TEXT ? XS_COPEN : s;
    case XC_LT_PI: return s == XS_TEXT ? XS_PI : s;
    case XC_LT_DECL: return s == XS_TEXT ? XS_DECL : s;
    case XC_GT: return (s == XS_TAG || s == XS_DECL) ? XS_TEXT : s;
    case XC_GT_DASH: return (s == XS_TAG || s == XS_DECL || s == XS_COMMENT) ? XS_TEXT : s;
    case XC_GT_BRK: return (s == XS_TAG || s == XS_DECL || s == XS_CDATA) ? XS_TEXT : s;
    case XC_GT_Q: return (s == XS_TAG || s == XS_DECL || s == XS_PI) ? XS_TEXT : s;
    case XC_DQ: return s == XS_TAG ? XS_DQ : (s == XS_DQ ? XS_TAG : s);
    case XC_SQ: return s == XS_TAG ? XS_SQ : (s == XS_SQ ? XS_TAG : s);
    case XC_LB: return s == XS_DECL ? XS_SUBSET : s;
    case XC_LB_CDATA: return s == XS_DECL ? XS_SUBSET : (s == XS_COPEN ? XS_CDATA : s);
    case XC_RB: return s == XS_SUBSET ? XS_DECL : s;
    default: return s;
    }
}
// the class as a packed map: field s (4 bits) = the state after a byte of the class in state s
constexpr uint64_t xml_map(uint32_t c) {
    uint64_t m = 0;
    for (uint32_t s = 0; s < 16; s++) m |= (uint64_t)(s < XS_N ? xml_step(s, c) : s) << (4 * s);
    return m;
}
constexpr uint64_t XML_ID = xml_map(XC_NONE);
__device__ const uint64_t XML_MAPS[16] = {xml_map(0), xml_map(1), xml_map(2), xml_map(3), xml_map(4), xml_map(5),
                                          xml_map(6), xml_map(7), xml_map(8), xml_map(9), xml_map(10), xml_map(11),
                                          xml_map(12), xml_map(13), xml_map(14), xml_map(15)};

struct XmlLds {                       // one wave's
    alignas(16) uint8_t in[16 + XML_STEP + 16];   // the step's bytes, the 16 before them, the 16 after them
    alignas(16) uint8_t out[16 + XML_STEP + 16];  // the carried tail (< 16 bytes), then the step's output
};
struct XmlShared {
    XmlLds w[XML_WAVES];
    uint64_t maps[16];
};
static_assert(sizeof(XmlShared) <= 20 * 1024, "at least the inflate kernel's 8 workgroups per CU");

// s -> g(f(s)): f first
__device__ __forceinline__ uint64_t xml_then(uint64_t f, uint64_t g) {
    uint64_t r = 0;
#pragma unroll
    for (uint32_t s = 0; s < XS_N; s++) {
        const uint32_t t = (uint32_t)(f >> (4 * s)) & 15u;
        r |= ((g >> (4 * t)) & 15ull) << (4 * s);
    }
    return r;
}
__device__ __forceinline__ uint32_t xml_apply(uint64_t f, uint32_t s) { return (uint32_t)(f >> (4 * s)) & 15u; }
__device__ __forceinline__ uint64_t xml_shfl_up(uint64_t x, uint32_t d) {
    return (uint64_t)__shfl_up((uint32_t)(x >> 32), d) << 32 | __shfl_up((uint32_t)x, d);
}

// 0x80 in each byte of w that equals c (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t xml_has(uint32_t w, uint32_t c) {
    const uint32_t x = w ^ (c * 0x01010101u);
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
// the four 0x80 marks of y as bits 0..3 (the products' bits 21..24 have one contributor each)
__device__ __forceinline__ uint32_t xml_nib(uint32_t y) { return (((y >> 7) * 0x00204081u) >> 21) & 15u; }

// The reference that starts with the '&' at row[a]: its input length n (0: none), m output bytes in ob
__device__ uint32_t xml_ref(const uint8_t *row, uint32_t a, uint32_t &m, uint32_t &ob) {
    const uint32_t c1 = row[a + 1], c2 = row[a + 2], c3 = row[a + 3];
    m = 1;
    if (c1 == '#') {
        const bool hex = (c2 | 0x20) == 'x';
        const uint32_t p = a + 2 + (hex ? 1u : 0u);
        uint32_t v = 0, nd = 0;
        for (; nd < 8; nd++) {
            const uint32_t d = row[p + nd];
            const int dv = hex ? dec_hexv(d) : (d - '0' < 10u ? (int)(d - '0') : -1);
            if (dv < 0) break;
            v = hex ? v << 4 | (uint32_t)dv : v * 10 + (uint32_t)dv;
        }
        if (nd == 0 || row[p + nd] != ';' || v == 0 || v > 0x10FFFF || (v >= 0xD800 && v <= 0xDFFF)) return 0;
        if (v < 0x80) ob = v;
        else if (v < 0x800) { m = 2; ob = (0xC0 | v >> 6) | (0x80 | (v & 63)) << 8; }
        else if (v < 0x10000) { m = 3; ob = (0xE0 | v >> 12) | (0x80 | (v >> 6 & 63)) << 8 | (0x80 | (v & 63)) << 16; }
        else { m = 4; ob = (0xF0 | v >> 18) | (0x80 | (v >> 12 & 63)) << 8 | (0x80 | (v >> 6 & 63)) << 16 | (0x80 | (v & 63)) << 24; }
        return p - a + nd + 1;
    }
    if (c2 == 't' && c3 == ';' && (c1 == 'l' || c1 == 'g')) { ob = c1 == 'l' ? '<' : '>'; return 4; }
    const uint32_t c4 = row[a + 4], c5 = row[a + 5];
    if (c1 == 'a' && c2 == 'm' && c3 == 'p' && c4 == ';') { ob = '&'; return 5; }
    if (c1 == 'q' && c2 == 'u' && c3 == 'o' && c4 == 't' && c5 == ';') { ob = '"'; return 6; }
    if (c1 == 'a' && c2 == 'p' && c3 == 'o' && c4 == 's' && c5 == ';') { ob = '\''; return 6; }
    return 0;
}

// the wave's output: the LDS row holds stream bytes [gpos, gpos + T) of the slot, where stream byte s
// lives at base[s] and base is 16-byte aligned; [dmis, limit) of the stream is the slot
struct XmlOut {
    uint8_t *base;
    uint32_t gpos, T, dmis, limit;
};
// the row's whole vectors (final: all of it) leave; the rest moves to the row's front
__device__ void xml_flush(XmlLds &W, XmlOut &O, uint32_t lane, bool final) {
    const uint32_t nv = final ? (O.T + 15) / 16 : O.T / 16;
    const uint32_t end = min(O.gpos + O.T, O.limit);
    for (uint32_t v = lane; v < nv; v += 64) {
        const uint32_t s0 = O.gpos + 16 * v;
        const uint4 q = *reinterpret_cast<const uint4 *>(W.out + 16 * v);
        if (s0 >= O.dmis && s0 + 16 <= end) {
            *reinterpret_cast<uint4 *>(O.base + s0) = q;
        } else {   // the slot's first or last vector
            const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (uint32_t k = 0; k < 16; k++)
                if (s0 + k >= O.dmis && s0 + k < end) O.base[s0 + k] = (uint8_t)(d[k >> 2] >> (8 * (k & 3)));
        }
    }
    if (final) return;
    const uint32_t rem = O.T - 16 * nv;
    const uint32_t t = lane < rem ? W.out[16 * nv + lane] : 0u;
    infl_sync();
    if (lane < rem) W.out[lane] = (uint8_t)t;
    O.gpos += 16 * nv;
    O.T = rem;
}

// The view of the body src[0, n) -> dst[0, <= n): its length, or GM_NONE.
__device__ uint32_t xml_body(XmlLds &W, const uint64_t *maps, const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t lane) {
    const uint32_t skew = (uint32_t)((uintptr_t)src & 15);
    const uint64_t total64 = (uint64_t)skew + n;
    if (n == 0 || total64 > 0x7FFFFF00u) return GM_NONE;   // (32-bit buffer offsets: no view of a body that long)
    const uint32_t total = (uint32_t)total64;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(src - skew), (short)0, (int)((total + 15) & ~15u), 0x00020000);
    XmlOut O;
    O.dmis = (uint32_t)((uintptr_t)dst & 15);
    O.base = dst - O.dmis;
    O.gpos = 0;
    O.T = O.dmis;
    O.limit = O.dmis + n;
    if (lane < 4) reinterpret_cast<uint32_t *>(W.in)[lane] = 0;   // nothing before the body
    uint32_t carry = XS_TEXT, carry_amp = 0;
    for (uint32_t r0 = 0; r0 < total; r0 += XML_STEP) {
        // ---- (1) load: w = resource bytes [off, off + 16), zero outside [skew, total)
        const uint32_t off = r0 + 16 * lane;
        uint32_t w[4], x[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) w[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(off + 4 * j), 0, 0);
        if (lane == 0) {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) x[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(r0 + XML_STEP + 4 * j), 0, 0);
        }
        const uint32_t vlo = skew > off ? min(skew - off, 16u) : 0u, vhi = total > off ? min(total - off, 16u) : 0u;
        const uint32_t vmask = ((1u << vhi) - 1) & ~((1u << vlo) - 1);   // the lane's bytes inside the body
        if (r0 == 0 || r0 + XML_STEP + 16 > total) {   // (wave-uniform: the body's first and last step)
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t b4 = (vmask >> (4 * j)) & 15u;
                w[j] &= (b4 & 1 ? 0xFFu : 0u) | (b4 & 2 ? 0xFF00u : 0u) | (b4 & 4 ? 0xFF0000u : 0u) | (b4 & 8 ? 0xFF000000u : 0u);
                const uint32_t xo = r0 + XML_STEP + 4 * j, xh = total > xo ? min(total - xo, 4u) : 0u;
                x[j] &= xh >= 4 ? 0xFFFFFFFFu : (1u << (8 * xh)) - 1;
            }
        }
        *reinterpret_cast<uint4 *>(W.in + 16 + 16 * lane) = make_uint4(w[0], w[1], w[2], w[3]);
        if (lane == 0) *reinterpret_cast<uint4 *>(W.in + 16 + XML_STEP) = make_uint4(x[0], x[1], x[2], x[3]);
        infl_sync();
        // ---- (2) the event bytes ('<' '>' '"' ''' '[' ']') and the '&' of the lane's sixteen, as bit masks
        uint32_t evm = 0, amp = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t ye = xml_has(w[j], '<') | xml_has(w[j], '>') | xml_has(w[j], '"') | xml_has(w[j], '\'') |
                                xml_has(w[j], '[') | xml_has(w[j], ']');
            evm |= xml_nib(ye) << (4 * j);
            amp |= xml_nib(xml_has(w[j], '&')) << (4 * j);
        }
        // each event's class from its neighbours in the row (cls16: field j = byte j's class; cdrop: a
        // byte of "]]>"), and (3) the lane's map composed on the way
        const uint8_t *row = W.in + 16 + 16 * lane;
        uint64_t cls16 = 0, f = XML_ID;
        uint32_t cdrop = 0;
        for (uint32_t m = evm; m; m &= m - 1) {
            const uint32_t j = (uint32_t)__builtin_ctz(m), c = row[j];
            uint32_t cls;
            if (c == '<') {
                const uint32_t n1 = row[j + 1];
                cls = XC_LT_TAG;
                if (n1 == '?') cls = XC_LT_PI;
                else if (n1 == '!') {
                    const uint32_t n2 = row[j + 2];
                    cls = XC_LT_DECL;
                    if (n2 == '-' && row[j + 3] == '-') cls = XC_LT_COMMENT;
                    else if (n2 == '[' && row[j + 3] == 'C' && row[j + 4] == 'D' && row[j + 5] == 'A' && row[j + 6] == 'T' &&
                             row[j + 7] == 'A' && row[j + 8] == '[')
                        cls = XC_LT_CDATA;
                }
            } else if (c == '>') {
                const uint32_t p1 = row[(int)j - 1], p2 = row[(int)j - 2];
                cls = p1 == '-' && p2 == '-' ? XC_GT_DASH : p1 == ']' && p2 == ']' ? XC_GT_BRK : p1 == '?' ? XC_GT_Q : XC_GT;
                if (cls == XC_GT_BRK) cdrop |= 1u << j;
            } else if (c == '"') cls = XC_DQ;
            else if (c == '\'') cls = XC_SQ;
            else if (c == '[') {
                cls = XC_LB;
                if (row[(int)j - 1] == 'A' && row[(int)j - 2] == 'T' && row[(int)j - 3] == 'A' && row[(int)j - 4] == 'D' &&
                    row[(int)j - 5] == 'C' && row[(int)j - 6] == '[' && row[(int)j - 7] == '!' && row[(int)j - 8] == '<')
                    cls = XC_LB_CDATA;
            } else {
                cls = XC_RB;
                const uint32_t n1 = row[j + 1];
                if ((n1 == ']' && row[j + 2] == '>') || (row[(int)j - 1] == ']' && n1 == '>')) cdrop |= 1u << j;
            }
            cls16 |= (uint64_t)cls << (4 * j);
            f = xml_then(f, maps[cls]);
        }
        // the wave's scan (skipped when no lane holds an event), the lane's start state
        uint64_t F = f;
        if (__ballot(evm != 0)) {
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint64_t G = xml_shfl_up(F, d);
                if (lane >= d) F = xml_then(G, F);
            }
        }
        const uint64_t E = xml_shfl_up(F, 1);
        const uint32_t st0 = lane == 0 ? carry : xml_apply(E, carry);
        const uint64_t Fall = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(F >> 32), 63) << 32 |
                              (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)F, 63);
        carry = xml_apply(Fall, carry);
        // ---- (4) references: each '&' in [x0 - 11, x0 + 16), bit i <-> byte x0 - 11 + i
        uint32_t pamp = __shfl_up(amp, 1);
        if (lane == 0) pamp = carry_amp;
        carry_amp = (uint32_t)__builtin_amdgcn_readlane((int)amp, 63);
        uint32_t win = amp << 11 | pamp >> 5, refmask = 0, refemit = 0;
        uint64_t ovl = 0, ovh = 0;   // the references' output bytes at their input positions
        while (win) {
            const uint32_t i = (uint32_t)__builtin_ctz(win);
            win &= win - 1;
            uint32_t m = 0, ob = 0;
            const uint32_t nref = xml_ref(W.in, 16 + 16 * lane + i - 11, m, ob);
            if (nref == 0) continue;
            // bit k of b <-> the reference's byte k; own byte j = k + i - 11
            const uint32_t bn = (1u << nref) - 1, bm = (1u << m) - 1;
            refmask |= (i >= 11 ? bn << (i - 11) : bn >> (11 - i)) & 0xFFFFu;
            refemit |= (i >= 11 ? bm << (i - 11) : bm >> (11 - i)) & 0xFFFFu;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t j = k + i - 11;   // (wraps below 0: >= 16)
                const uint64_t b = (uint64_t)((ob >> (8 * k)) & 0xFFu) << (8 * (j & 7));
                if (k < m && j < 8) ovl |= b;
                if (k < m && j >= 8 && j < 16) ovh |= b;
            }
        }
        // ---- the replay, event by event: the state holds over the run of bytes before each event.
        // emask: the bytes emitted; chrm: the bytes whose state is character data; a '\n' goes into
        // the output bytes (obl: bytes 0..7, obh: 8..15) in place of a tag's '<' or a closing quote
        const uint32_t chrkeep = ~(refmask & ~refemit), cdkeep = ~cdrop;
        uint32_t st = st0, emask = 0, chrm = 0, prev = 0;
        uint64_t obl = (uint64_t)w[1] << 32 | w[0], obh = (uint64_t)w[3] << 32 | w[2];
        for (uint64_t ev = cls16; ev;) {
            const uint32_t sh = (uint32_t)__builtin_ctzll(ev) & ~3u, j = sh >> 2, cls = (uint32_t)(ev >> sh) & 15u;
            ev &= ~(15ull << sh);
            const uint32_t bit = 1u << j, run = (bit - 1) & ~((1u << prev) - 1);
            const bool chr = st == XS_TEXT || st == XS_DQ || st == XS_SQ;
            emask |= run & (chr ? chrkeep : st == XS_CDATA ? cdkeep : 0u);
            if (chr) chrm |= run;
            const bool lt = cls >= XC_LT_TAG && cls <= XC_LT_DECL;
            if ((st == XS_TEXT && cls == XC_LT_TAG) || (st == XS_DQ && cls == XC_DQ) || (st == XS_SQ && cls == XC_SQ)) {
                emask |= bit;
                const uint64_t fm = 0xFFull << (8 * (j & 7)), nl = (uint64_t)'\n' << (8 * (j & 7));
                if (j < 8) obl = (obl & ~fm) | nl; else obh = (obh & ~fm) | nl;
            } else if (chr && !(st == XS_TEXT && lt)) {
                emask |= bit;   // (an event byte lies in no reference)
            } else if (st == XS_CDATA) {
                emask |= bit & cdkeep;
            }
            st = xml_apply(maps[cls], st);
            prev = j + 1;
        }
        {
            const uint32_t run = 0xFFFFu & ~((1u << prev) - 1);
            const bool chr = st == XS_TEXT || st == XS_DQ || st == XS_SQ;
            emask |= run & (chr ? chrkeep : st == XS_CDATA ? cdkeep : 0u);
            if (chr) chrm |= run;
        }
        // a reference in character data: its output bytes in place of its first input bytes
        for (uint32_t m = refemit & chrm; m; m &= m - 1) {
            const uint32_t j = (uint32_t)__builtin_ctz(m);
            const uint64_t fm = 0xFFull << (8 * (j & 7));
            if (j < 8) obl = (obl & ~fm) | (ovl & fm); else obh = (obh & ~fm) | (ovh & fm);
        }
        emask &= vmask;
        // ---- (5) compaction into the output row, whole vectors out
        const uint32_t cnt = (uint32_t)__popc(emask);
        uint32_t pre = cnt;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(pre, d);
            if (lane >= d) pre += t;
        }
        const uint32_t sum = (uint32_t)__builtin_amdgcn_readlane((int)pre, 63);
        uint32_t pos = O.T + pre - cnt;
        if (emask == 0xFFFFu) {   // (plain text: the sixteen bytes as they are)
#pragma unroll
            for (uint32_t j = 0; j < 16; j++) W.out[pos + j] = (uint8_t)((j < 8 ? obl : obh) >> (8 * (j & 7)));
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 16; j++)
                if (emask >> j & 1) W.out[pos++] = (uint8_t)((j < 8 ? obl : obh) >> (8 * (j & 7)));
        }
        O.T += sum;
        infl_sync();   // (also: the input row's reads above before the writes below and the next step's)
        if (lane == 63) *reinterpret_cast<uint4 *>(W.in) = make_uint4(w[0], w[1], w[2], w[3]);
        xml_flush(W, O, lane, false);
    }
    infl_sync();
    xml_flush(W, O, lane, true);
    return min(O.gpos + O.T, O.limit) - O.dmis;
}

// whether the request's body is taken: "xml" in the first Content-Type value, or the "<?xml" prolog
__device__ bool xml_selected(const uint8_t *A, const Rec &r, uint64_t hdrs, uint64_t body) {
    HdrIt it{hdrs, hdrs + r.hdr_len};
    uint64_t ns, vs; uint32_t nl, vl;
    const uint8_t ct[13] = "content_type";
    while (hdr_next(A, it, ns, nl, vs, vl)) {
        if (!hdr_name_is(A, ns, nl, ct, 12)) continue;
        for (uint32_t k = 0; k + 3 <= vl; k++)
            if (lc(A[vs + k]) == 'x' && lc(A[vs + k + 1]) == 'm' && lc(A[vs + k + 2]) == 'l') return true;
        break;
    }
    const uint8_t *b = A + body;
    uint32_t p = 0;
    if (r.body_len >= 3 && b[0] == 0xEF && b[1] == 0xBB && b[2] == 0xBF) p = 3;
    while (p < r.body_len && (b[p] == ' ' || b[p] == '\t' || b[p] == '\r' || b[p] == '\n')) p++;
    return p + 5 <= r.body_len && b[p] == '<' && b[p + 1] == '?' && b[p + 2] == 'x' && b[p + 3] == 'm' && b[p + 4] == 'l';
}

__global__ void k_xml_reset(uint32_t *__restrict__ ctl) {
    if (threadIdx.x < XML_CTL_WORDS) ctl[threadIdx.x] = 0;
}

// lim[i] = the slot of request i (its body_len; 0: not an XML body, or -- with verdicts -- its
// location does not run the parser), len_out[i] = GM_NONE, the XML bodies' indices appended to list
__global__ void k_xml_size(const gm_req *__restrict__ reqs, const uint8_t *__restrict__ A, uint64_t alen,
                           const uint64_t *__restrict__ dlen, uint32_t n, const gm_verdict *__restrict__ verdicts,
                           const DLocUri *__restrict__ loc_uri, uint32_t n_locs, uint64_t *__restrict__ lim,
                           uint32_t *__restrict__ len_out, uint32_t *__restrict__ list, uint32_t *__restrict__ ctl) {
    const uint64_t len = dlen ? min(*dlen, alen) : alen;
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t i0 = blockIdx.x * blockDim.x; i0 < n; i0 += gridDim.x * blockDim.x) {
        const uint32_t i = i0 + threadIdx.x;
        bool xml = false;
        if (i < n) {
            bool run = true;
            if (verdicts) {
                const gm_verdict v = verdicts[i];
                run = waf_active(v) && v.location_id < n_locs && ((loc_uri[v.location_id].flags >> LOCURI_DEC_SHIFT) & DEC_XML);
            }
            uint64_t l = 0;
            if (run) {
                const Rec r = load_rec(reqs + i);
                const uint64_t hdrs = r.base + r.uri_len + r.args_len, body = hdrs + r.hdr_len;
                if (r.body_len && body + r.body_len <= len && xml_selected(A, r, hdrs, body)) {
                    xml = true;
                    l = r.body_len;
                }
            }
            lim[i] = l;
            len_out[i] = GM_NONE;
            if (i + 1 == n) lim[n] = 0;
        }
        const unsigned long long m = __ballot(xml);
        if (m) {
            uint32_t b = 0;
            if (lane == (uint32_t)__builtin_ctzll(m)) b = atomicAdd(ctl, (uint32_t)__popcll(m));
            b = __shfl(b, __builtin_ctzll(m));
            if (xml) list[b + mp_rank(m)] = i;
        }
    }
}

// persistent workgroups: each wave pulls the next listed body and writes its view to out[off[i] ...)
__global__ __launch_bounds__(XML_BLOCK) __attribute__((amdgpu_waves_per_eu(4))) void k_xml(const gm_req *__restrict__ reqs, const uint8_t *__restrict__ A, uint32_t n,
                                                   const uint32_t *__restrict__ list, uint32_t *__restrict__ ctl,
                                                   uint8_t *__restrict__ out, uint64_t out_cap,
                                                   const uint64_t *__restrict__ off, uint32_t *__restrict__ len_out,
                                                   uint32_t *__restrict__ views, uint32_t *__restrict__ ov) {
    __shared__ XmlShared sh;
    if (threadIdx.x < 16) sh.maps[threadIdx.x] = XML_MAPS[threadIdx.x];
    __syncthreads();
    XmlLds &W = sh.w[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t m = min(infl_u(ctl[0]), n);
    // As in k_multipart: one back edge, no lane-divergent branch at the loop's level.  (At least four
    // waves per SIMD asked of the compiler: without a cap an earlier form of the step took 246 VGPRs.)
    for (;;) {
        const uint32_t q = infl_u(atomicAdd(ctl + 1, lane == 0 ? 1u : 0u));   // (lane 0: the value before the wave's add)
        if (q >= m) break;
        const uint32_t i = min(infl_u(list[q]), n - 1);
        const Rec r = load_rec(reqs + i);
        const uint32_t blen = infl_u(r.body_len);
        const uint8_t *src = A + uniform64(r.base + r.uri_len + r.args_len + r.hdr_len);
        const uint64_t o = uniform64(off[i]);
        const bool fits = o + blen <= out_cap;
        uint32_t res = GM_NONE;
        if (fits) res = infl_u(xml_body(W, sh.maps, src, blen, out + o, lane));
        len_out[i] = res;   // (the same word from every lane: one store)
        atomicAdd(views, lane == 0 && res != GM_NONE ? 1u : 0u);
        atomicOr(ov, lane == 0 && !fits ? 1u : 0u);
    }
}
