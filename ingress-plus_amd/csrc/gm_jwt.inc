// gm_jwt.inc -- HS256, RS256 and ES256 JWT verification for `auth_jwt` locations (NGINX Plus; nginx-plus.ingress.tmpl
// :105-111,186-188,223-228), included into gm_device.hip's anonymous namespace: gm_auth_jwt's kernels.
//
// THE GRAMMAR (include/gpumatch.h states the same; tests/jwt_reference.py restates it in Python).
// Which requests.  The verdict's action is GM_ACT_PROXY or GM_ACT_BLOCK and its location carries an
//   auth record (DAuth); every other request answers GM_AUTH_NONE.  A verdict of another generation
//   (or a record that leaves the arena) answers GM_AUTH_DEFER / GM_AUTH_R_STALE.
// Token text.  The source's value: the first Authorization header's (it must begin with "Bearer",
//   ASCII case-insensitively, and one space; further spaces are skipped), or the value of the
//   cookie, argument or header that `token=$cookie_NAME | $arg_NAME | $http_NAME` names, as nginx's
//   variables read them.  The token is the value's bytes up to its first space or its end; none, or
//   an empty one: DENY / NO_TOKEN.  It must be exactly three non-empty segments of [A-Za-z0-9_-]
//   split by two '.', with no padding; segment 3 is 43 characters (32 bytes) -- or, where the
//   location's key set holds an RSA key, 342, 512 or 683 (256, 384, 512 bytes), or, where it holds an EC
//   key, 86 (r | s, 64 bytes); a segment of 4k + 1
//   characters decodes to nothing.  Anything else: DENY / MALFORMED.
// Header and payload.  Each decodes as base64url to one JSON object (whitespace around it allowed,
//   nothing else).  Only top-level members are read, the last of a repeated name winning:
//     alg   a string: "HS256" goes on, "RS256" where the set holds an RSA key, "ES256" where it holds an EC key; "none" is DENY /
//           ALG_NONE, any other value (one written with an escape included) DEFER / ALG; missing or
//           not a string: MALFORMED.
//     kid   a string, optional (anything else there is ignored).
//     exp, nbf   optional; a JSON integer ('-'? and 1..18 digits, nothing after them) or a string of
//           1..18 decimal digits.  Anything else there: MALFORMED.
//   Every other value is skipped: strings with their escapes honoured, objects and arrays by depth.
//   A member name that holds a backslash is MALFORMED (deviation: nginx would unescape it; failing
//   closed keeps an escaped "exp" from going unread).
// Candidate keys.  The set's keys of the alg's kind -- `oct` for HS256, RSA for RS256, EC (P-256) for ES256; an
//   RSA or EC key is never an HMAC key -- whose kid equals the token's, byte for byte, if the token has a kid and some
//   key of that kind has that one; otherwise all keys of the kind (at most GM_JWT_KEYS in a set, of
//   all kinds together).  None of the kind: DENY / SIGNATURE.
// Accept.  Some candidate key verifies (else DENY / SIGNATURE).  HS256: segment 3 is 43 characters
//   (else MALFORMED) and HMAC-SHA-256(key, segment1 "." segment2 as sent) equals its 32 bytes.
//   RS256, a key whose modulus n is k bytes (256, 384, 512; e = 65537): segment 3 is ceil(4k / 3)
//   characters; its first 8k bits, a big-endian integer s, are < n (surplus bits ignored, as for
//   HS256); and s^65537 mod n equals, over all k bytes, the EMSA-PKCS1-v1_5 encoding
//   00 01 FF..FF 00 | 30 31 30 0d 06 09 60 86 48 01 65 03 04 02 01 05 00 04 20 | SHA-256(segment1 "."
//   segment2) -- nothing inside the padding is parsed.
//   ES256 (group order n): segment 3 is 86 characters (HS256 with 86: MALFORMED; ES256 with another admitted
//   length, RS256 with 86: SIGNATURE); its first 512 bits are r | s, big-endian, 1 <= r, s < n (the 4 surplus
//   bits ignored); e = SHA-256(segment1 "." segment2), w = 1 / s, u1 = e w, u2 = r w (mod n), R = u1 G + u2 Q:
//   R is not the point at infinity and x_R mod n = r.  High s is accepted.  A set without an EC key answers
//   every input as before ES256 was known.  Then exp + leeway > now (else DENY / EXPIRED)
//   and nbf <= now + leeway (else DENY / NOT_YET).  Claims are read only of a token whose signature
//   verified, so a forged token is always SIGNATURE, whatever its payload.
//
// WORK SPLIT.
// k_jwt_find   a lane per request: the auth record, the token's span (the span helpers of the rules
//   path), its shape, the header's alg and kid -- read from a streaming base64url reader, no
//   scratch -- and the signature's eight big-endian words.  A request decided here writes out_auth;
//   the others leave a work item and count themselves into a histogram over SHA block counts
//   ceil((len + 9) / 64), one atomic per (wave, bin).
// k_jwt_order  the counting sort's scatter: order[] lists the work items by block count, so the 64
//   tokens of a k_jwt_hmac wave are of like length (unsorted, a wave runs as long as its longest).
// k_jwt_hmac   the hot path: a lane per token.  The eight state words and the sixteen-word message
//   schedule live in VGPRs through the 64 fully unrolled rounds (the round constants are literals);
//   rotates are v_alignbit_b32.  The text is read with dword-aligned loads -- the lane's own
//   contiguous 64-byte run per block, both halves of a 128-byte line used by consecutive blocks --
//   and ONE v_perm_b32 per word both undoes the text's byte offset in the arena and makes the word
//   big-endian (selector 0x00010203 + 0x01010101 * (offset & 3) over the dword pair).  A full block
//   reads one dword past its 64 bytes; that dword lies in the token ('.' and the 43 signature
//   characters follow the signing input).  The tail blocks are built from the length, loading only
//   dwords that hold a text byte, so nothing outside the token's aligned dwords is read.  The inner
//   hash starts from the key's precomputed inner midstate and the outer hash is one compress of
//   digest | padding from the outer midstate: blocks + 2 compresses per token.  A lane whose first
//   candidate key fails goes round again with the next one (rare).  The compare ORs the XORs of all
//   eight words: no early exit.  An RS256 token runs in the same sorted launch as plain SHA-256 from
//   the IV (no key block before it, no outer compress): its lane leaves the digest where an HS256
//   token's signature words are and lists itself by modulus size, one atomic per (wave, size).
// k_jwt_rsa<K> RS256's hot path, a launch per modulus size present (K = 64, 96, 128 limbs of 32 bits)
//   over that size's list: a lane per token, 64-thread groups.  s^65537 mod n is 18 Montgomery
//   products -- s * RR, sixteen squarings, * s (which also leaves Montgomery form) -- each K fused
//   CIOS rows: row i adds a_i * b and m * n (m = t_0 * -1/n mod 2^32) into the accumulator t and
//   shifts it down a limb.  The multiplicand b[K] and t[K + 1] live in VGPRs, the loop over the K
//   limbs of a row fully unrolled so every register index is static: per limb two 32 x 32 + 64 bit
//   multiply-adds (v_mad_u64_u32), the carries of both chains folded into the addends.  The rows are
//   a real loop, so the multiplier a is read at a dynamic index: it lives in LDS, limb i of lane l at
//   word 64 i + l (conflict-free; one ds_read_b32 per row, K ds_write_b32 per product) -- 16, 24 or
//   32 KiB a wave and no other LDS.  n is read through the key pointer, four limbs a load (the lanes
//   of a wave nearly always share the key: one line a load); for K = 64 it is held in VGPRs too.
//   A conditional subtract per product keeps y < n.  The signature is decoded by the lane from the
//   token's own characters (the last characters are limb 0) straight into LDS, and checked < n on the
//   way; for the last product it is decoded again (a = s, b = y: LDS held y by then).  The compare
//   ORs the XORs of all K limbs against the encoding built from the digest: no early exit.
// k_jwt_ec    ES256's hot path, one launch where the generation has a P-256 key, over the fourth list (an ES256
//   token hashes like an RS256 one and lists itself as class 3): a lane per token, 64-thread groups, the whole
//   verification in VGPRs and no LDS (gm_p256.hpp).  Field elements are eight 32-bit limbs in Montgomery form;
//   p = -1 mod 2^32 makes the reduction of a row three adds and a subtract of the low limb, so a field product
//   is 64 v_mad_u64_u32 and carry chains.  1 / s mod n is a fixed chain over generic 8-limb CIOS products.
//   u1 G + u2 Q is Shamir's trick over joint 2-bit windows: 128 steps of two Jacobian doublings (a = -3) and
//   one mixed addition of the key's table entry i G + j Q (the compiler wrote all 15, affine, Montgomery form:
//   four dwordx4 loads through the key pointer), a (0, 0) window dropped by select.  The addition handles an
//   accumulator at infinity (select), an addend equal to it (a doubling, under a branch) and opposite to it
//   (Z = 0 falls out of the formula); Z = 0 at the end is refused before the compare r Z^2 = X or (r + n) Z^2
//   = X, which needs no inversion and ORs the XORs of all limbs.
// k_jwt_claims a lane per verified token, in the same order: exp / nbf from the payload through the
//   streaming reader, then out_auth.

constexpr uint32_t JWT_BINS = 64;   // block counts 1 .. 63, and 64 or more
// control words of one launch: [0] work items, [2 ..) the histogram, then the scatter's cursors
// and the RS256 tokens of each modulus size
constexpr uint32_t JWT_CTL_HIST = 2, JWT_CTL_CUR = JWT_CTL_HIST + JWT_BINS, JWT_CTL_RSA = JWT_CTL_CUR + JWT_BINS,
                   JWT_CTL_WORDS = JWT_CTL_RSA + 4;
// item0.x: the SHA block count, and above it
constexpr uint32_t JWT_VERIFIED = 0x80000000u;   // k_jwt_hmac / k_jwt_rsa verified the signature
constexpr uint32_t JWT_RSA = 0x40000000u;        // an RS256 token, its modulus size class (0 .. 2) at JWT_CLS_SHIFT,
constexpr uint32_t JWT_CLS_EC = 3;               // or an ES256 token: class 3 (both hash as plain SHA-256)
constexpr uint32_t JWT_CLS_SHIFT = 28, JWT_NB_MASK = (1u << JWT_CLS_SHIFT) - 1;

struct JwtTab {
    const DAuth *auth;       // per location; nullptr: the generation has no auth record
    const DJwk *keys;
    const uint8_t *bytes;
    uint32_t n_locs, gen;
    const uint32_t *limbs;   // the RSA keys' n and RR, the EC keys' tables (DJwk.limb_off)
};

__device__ __forceinline__ uint32_t jwt_code(uint32_t code, uint32_t reason) { return code | reason << 8; }
__device__ __forceinline__ bool jwt_b64ok(uint32_t c) {
    return (c | 0x20) - 'a' < 26u || c - '0' < 10u || c == '-' || c == '_';
}
__device__ __forceinline__ uint32_t jwt_b64v(uint32_t c) {   // (of a character jwt_b64ok admits)
    return c >= 'a' ? c - 'a' + 26 : c == '_' ? 63u : c >= 'A' ? c - 'A' : c >= '0' ? c - '0' + 52 : 62u;
}

// the bytes a base64url segment decodes to, one at a time: cur is the byte at the cursor, -1 past the end
struct JwtRd {
    const uint8_t *p;
    uint32_t n, cp, acc, have;
    int cur;
    __device__ void init(const uint8_t *q, uint32_t len) { p = q; n = len; cp = 0; acc = 0; have = 0; adv(); }
    __device__ void adv() {
        if (have == 0) {
            const uint32_t rem = n - cp;
            if (rem < 2) { cur = -1; return; }
            const uint32_t k = min(rem, 4u);
            acc = 0;
            for (uint32_t j = 0; j < k; j++) acc |= jwt_b64v(p[cp + j]) << (18 - 6 * j);
            cp += k;
            have = k - 1;
        }
        cur = (int)((acc >> 16) & 0xFFu);
        acc <<= 8;
        have--;
    }
};

enum : uint32_t { JALG_MISSING, JALG_HS256, JALG_NONE, JALG_OTHER, JALG_BAD, JALG_RS256, JALG_ES256 };
struct JwtDoc {
    uint32_t alg, kid_mask;
    bool has_kid, has_exp, has_nbf;
    long long exp, nbf;
};

__device__ __forceinline__ bool jwt_is_ws(int c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
__device__ void jwt_ws(JwtRd &r) { while (jwt_is_ws(r.cur)) r.adv(); }
// the rest of a string whose opening quote is behind the cursor
__device__ bool jwt_skip_str(JwtRd &r) {
    for (;;) {
        const int c = r.cur;
        if (c < 0) return false;
        r.adv();
        if (c == '"') return true;
        if (c == '\\') { if (r.cur < 0) return false; r.adv(); }
    }
}
__device__ bool jwt_skip_val(JwtRd &r) {
    int c = r.cur;
    if (c < 0) return false;
    if (c == '"') { r.adv(); return jwt_skip_str(r); }
    if (c == '{' || c == '[') {
        for (uint32_t depth = 0;;) {
            c = r.cur;
            if (c < 0) return false;
            r.adv();
            if (c == '"') { if (!jwt_skip_str(r)) return false; }
            else if (c == '{' || c == '[') depth++;
            else if ((c == '}' || c == ']') && --depth == 0) return true;
        }
    }
    uint32_t k = 0;   // a number or a literal: up to the delimiter
    for (; (c = r.cur) >= 0 && c != ',' && c != '}' && c != ']' && !jwt_is_ws(c); k++) r.adv();
    return k > 0;
}
// exp / nbf: a JSON integer, or a string of 1..18 decimal digits
__device__ bool jwt_time(JwtRd &r, long long &v) {
    const bool str = r.cur == '"';
    if (str) r.adv();
    bool neg = false;
    if (!str && r.cur == '-') { neg = true; r.adv(); }
    uint32_t nd = 0;
    unsigned long long x = 0;
    for (; r.cur >= '0' && r.cur <= '9'; r.adv()) {
        if (++nd > 18) return false;
        x = x * 10 + (uint32_t)(r.cur - '0');
    }
    if (nd == 0) return false;
    if (str) { if (r.cur != '"') return false; r.adv(); }
    else if (!(r.cur < 0 || r.cur == ',' || r.cur == '}' || jwt_is_ws(r.cur))) return false;   // 1.5, 1e3
    v = neg ? -(long long)x : (long long)x;
    return true;
}
// the kid's value (the opening quote behind the cursor) against the set's kids: the keys that equal it
__device__ bool jwt_kid(JwtRd &r, const JwtTab &t, const DAuth &a, uint32_t &mask) {
    mask = (1u << a.n_keys) - 1;
    uint32_t j = 0;
    for (;; j++) {
        const int c = r.cur;
        if (c < 0) return false;
        r.adv();
        if (c == '"') break;
        if (c == '\\') { if (r.cur < 0) return false; r.adv(); mask = 0; continue; }   // (an escaped kid equals none)
        for (uint32_t k = 0; k < a.n_keys; k++) {
            const DJwk &K = t.keys[a.first_key + k];
            if ((mask >> k & 1) && (K.kid_len == GM_NONE || j >= K.kid_len || t.bytes[K.kid_off + j] != (uint32_t)c)) mask &= ~(1u << k);
        }
    }
    for (uint32_t k = 0; k < a.n_keys; k++) if (t.keys[a.first_key + k].kid_len != j) mask &= ~(1u << k);
    return true;
}
// the alg's value (the opening quote behind the cursor)
__device__ bool jwt_alg(JwtRd &r, uint32_t &alg) {
    uint32_t v0 = 0, v1 = 0, l = 0;
    bool esc = false;
    for (;; l++) {
        const int c = r.cur;
        if (c < 0) return false;
        r.adv();
        if (c == '"') break;
        if (c == '\\') { if (r.cur < 0) return false; r.adv(); esc = true; continue; }
        if (l < 4) v0 |= (uint32_t)c << (8 * l); else if (l < 8) v1 |= (uint32_t)c << (8 * (l - 4));
    }
    alg = esc ? JALG_OTHER : l == 5 && v0 == 0x35325348u && v1 == '6' ? JALG_HS256 : l == 5 && v0 == 0x35325352u && v1 == '6' ? JALG_RS256 :
          l == 5 && v0 == 0x35325345u && v1 == '6' ? JALG_ES256 :
          l == 4 && v0 == 0x656E6F6Eu ? JALG_NONE : JALG_OTHER;
    return true;
}
// one JSON object's top-level members: alg and kid of a header, exp and nbf of a payload
__device__ bool jwt_walk(JwtRd &r, bool hdr, const JwtTab &t, const DAuth &a, JwtDoc &d) {
    d.alg = JALG_MISSING; d.kid_mask = 0; d.has_kid = d.has_exp = d.has_nbf = false; d.exp = d.nbf = 0;
    jwt_ws(r);
    if (r.cur != '{') return false;
    r.adv();
    jwt_ws(r);
    if (r.cur == '}') r.adv();
    else for (;;) {
        jwt_ws(r);
        if (r.cur != '"') return false;
        r.adv();
        uint32_t nm = 0, nl = 0;
        for (;; nl++) {
            const int c = r.cur;
            if (c < 0 || c == '\\') return false;
            r.adv();
            if (c == '"') break;
            if (nl < 4) nm |= (uint32_t)c << (8 * nl);
        }
        jwt_ws(r);
        if (r.cur != ':') return false;
        r.adv();
        jwt_ws(r);
        const uint32_t key = nl == 3 ? nm : 0u;
        const bool str = r.cur == '"';
        if (hdr && key == 0x00676C61u) {          // "alg"
            if (str) { r.adv(); if (!jwt_alg(r, d.alg)) return false; }
            else { d.alg = JALG_BAD; if (!jwt_skip_val(r)) return false; }
        } else if (hdr && key == 0x0064696Bu) {   // "kid"
            d.has_kid = str;
            if (str) { r.adv(); if (!jwt_kid(r, t, a, d.kid_mask)) return false; }
            else if (!jwt_skip_val(r)) return false;
        } else if (!hdr && key == 0x00707865u) {  // "exp"
            if (!jwt_time(r, d.exp)) return false;
            d.has_exp = true;
        } else if (!hdr && key == 0x0066626Eu) {  // "nbf"
            if (!jwt_time(r, d.nbf)) return false;
            d.has_nbf = true;
        } else if (!jwt_skip_val(r)) return false;
        jwt_ws(r);
        const int c = r.cur;
        if (c != ',' && c != '}') return false;
        r.adv();
        if (c == '}') break;
    }
    jwt_ws(r);
    return r.cur < 0;
}

// One atomic per (wave, bin): every lane of the wave calls it; a lane that is `on` gets its slot
// in its bin, the value of ctr[bin] before the wave's add plus its rank among the wave's lanes there.
__device__ uint32_t jwt_bin_add(uint32_t *ctr, uint32_t bin, bool on) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t res = 0;
    for (unsigned long long todo = __ballot(on); todo;) {
        const int lead = __builtin_ctzll(todo);
        const uint32_t b = (uint32_t)__shfl((int)bin, lead);
        const bool mine = on && bin == b;
        const unsigned long long same = __ballot(mine);
        uint32_t base = 0;
        if (lane == (uint32_t)lead) base = atomicAdd(ctr + b, (uint32_t)__popcll(same));
        base = (uint32_t)__shfl((int)base, lead);
        if (mine) res = base + mp_rank(same);
        todo &= ~same;
    }
    return res;
}

__global__ void k_jwt_reset(uint32_t *__restrict__ ctl) {
    for (uint32_t k = threadIdx.x; k < JWT_CTL_WORDS; k += blockDim.x) ctl[k] = 0;
}

// Request i's outcome if it is decided here, else GM_NONE with its work item and signature written.
__device__ uint32_t jwt_find(const uint8_t *A, uint64_t len, const gm_req *rp, const JwtTab &t, const DAuth &a,
                             uint4 &it0, uint4 &it1, uint32_t *sig) {
    const Rec r = load_rec(rp);
    const uint64_t args = r.base + r.uri_len, hdrs = args + r.args_len;
    if (hdrs + r.hdr_len > len) return jwt_code(GM_AUTH_DEFER, GM_AUTH_R_STALE);
    uint64_t vo = 0;
    uint32_t vl = 0;
    bool f;
    const uint8_t *nm = t.bytes + a.name_off;
    if (a.src == AUTH_SRC_BEARER) {
        const uint8_t az[14] = "authorization", be[7] = "bearer";
        f = span_http(A, hdrs, r.hdr_len, az, 13, vo, vl) && vl >= 7 && A[vo + 6] == ' ';
        for (uint32_t k = 0; f && k < 6; k++) f = lc(A[vo + k]) == be[k];
        if (f) for (vo += 6, vl -= 6; vl && A[vo] == ' '; vo++, vl--) {}
    } else if (a.src == SRC_COOKIE) f = span_cookie(A, hdrs, r.hdr_len, nm, a.name_len, vo, vl);
    else if (a.src == SRC_ARG) f = span_arg(A, args, r.args_len, nm, a.name_len, vo, vl);
    else f = span_http(A, hdrs, r.hdr_len, nm, a.name_len, vo, vl);
    uint32_t tl = 0;
    if (f) while (tl < vl && A[vo + tl] != ' ') tl++;
    if (!f || tl == 0) return jwt_code(GM_AUTH_DENY, GM_AUTH_R_NO_TOKEN);
    const uint8_t *T = A + vo;
    uint32_t d1 = GM_NONE, d2 = GM_NONE;
    for (uint32_t k = 0; k < tl; k++) {
        const uint32_t c = T[k];
        if (c == '.') {
            if (d1 == GM_NONE) d1 = k; else if (d2 == GM_NONE) d2 = k; else return jwt_code(GM_AUTH_DENY, GM_AUTH_R_MALFORMED);
        } else if (!jwt_b64ok(c)) return jwt_code(GM_AUTH_DENY, GM_AUTH_R_MALFORMED);
    }
    const uint32_t sl = tl - d2 - 1;   // segment 3 (if there is one)
    const bool sl_ok = sl == 43 || (a.rsa_mask && (sl == jwt_rsa_chars(JWT_RSA_K0) || sl == jwt_rsa_chars(JWT_RSA_K1) || sl == jwt_rsa_chars(JWT_RSA_K2))) ||
                       (a.ec_mask && sl == JWT_EC_CHARS);
    if (d2 == GM_NONE || d1 == 0 || d2 == d1 + 1 || !sl_ok || (d1 & 3) == 1 || ((d2 - d1 - 1) & 3) == 1)
        return jwt_code(GM_AUTH_DENY, GM_AUTH_R_MALFORMED);
    JwtRd rd;
    JwtDoc d;
    rd.init(T, d1);
    if (!jwt_walk(rd, true, t, a, d) || d.alg == JALG_MISSING || d.alg == JALG_BAD) return jwt_code(GM_AUTH_DENY, GM_AUTH_R_MALFORMED);
    if (d.alg == JALG_NONE) return jwt_code(GM_AUTH_DENY, GM_AUTH_R_ALG_NONE);
    const uint32_t slen = d2, all = (1u << a.n_keys) - 1;   // slen: segment1 "." segment2
    if (d.alg == JALG_ES256 && a.ec_mask) {
        // the EC keys, narrowed by kid; r | s stay in the text
        if (sl != JWT_EC_CHARS) return jwt_code(GM_AUTH_DENY, GM_AUTH_R_SIGNATURE);
        uint32_t cand = all & a.ec_mask;
        if (d.has_kid && (d.kid_mask & cand)) cand &= d.kid_mask;
        it0 = make_uint4((slen + 9 + 63) / 64 | JWT_RSA | JWT_CLS_EC << JWT_CLS_SHIFT, slen, (uint32_t)vo, (uint32_t)(vo >> 32));
        it1 = make_uint4(a.first_key, cand, d1 + 1, a.leeway);
        return GM_NONE;
    }
    if (d.alg == JALG_RS256 && a.rsa_mask) {
        if (sl == JWT_EC_CHARS) return jwt_code(GM_AUTH_DENY, GM_AUTH_R_SIGNATURE);   // (no RSA key of that size)
        // the RSA keys, narrowed by kid, that are of the size segment 3 has; the signature stays in the text
        uint32_t cand = all & a.rsa_mask, fit = 0;
        if (d.has_kid && (d.kid_mask & cand)) cand &= d.kid_mask;
        const uint32_t cls = sl == jwt_rsa_chars(JWT_RSA_K0) ? 0u : sl == jwt_rsa_chars(JWT_RSA_K1) ? 1u : 2u;
        for (uint32_t k = 0; k < a.n_keys; k++)
            if ((cand >> k & 1) && sl != 43 && t.keys[a.first_key + k].limbs == jwt_rsa_k(cls)) fit |= 1u << k;
        if (!fit) return jwt_code(GM_AUTH_DENY, GM_AUTH_R_SIGNATURE);
        it0 = make_uint4((slen + 9 + 63) / 64 | JWT_RSA | cls << JWT_CLS_SHIFT, slen, (uint32_t)vo, (uint32_t)(vo >> 32));
        it1 = make_uint4(a.first_key, fit, d1 + 1, a.leeway);
        return GM_NONE;
    }
    if (d.alg != JALG_HS256) return jwt_code(GM_AUTH_DEFER, GM_AUTH_R_ALG);
    if (sl != 43) return jwt_code(GM_AUTH_DENY, GM_AUTH_R_MALFORMED);
    uint32_t cand = all & ~a.rsa_mask & ~a.ec_mask;
    if (!cand) return jwt_code(GM_AUTH_DENY, GM_AUTH_R_SIGNATURE);
    if (d.has_kid && (d.kid_mask & cand)) cand &= d.kid_mask;
    // segment 3: 43 characters = 258 bits, the first 256 of them as eight big-endian words
    unsigned long long acc = 0;
    for (uint32_t k = 0, bits = 0, wi = 0; k < 43; k++) {
        acc = acc << 6 | jwt_b64v(T[d2 + 1 + k]);
        bits += 6;
        if (bits >= 32) { bits -= 32; sig[wi++] = (uint32_t)(acc >> bits); }
    }
    it0 = make_uint4((slen + 9 + 63) / 64, slen, (uint32_t)vo, (uint32_t)(vo >> 32));
    it1 = make_uint4(a.first_key, cand, d1 + 1, a.leeway);
    return GM_NONE;
}

__global__ __launch_bounds__(256) void k_jwt_find(const gm_req *__restrict__ reqs, const uint8_t *__restrict__ A,
                                                  uint64_t alen, const uint64_t *__restrict__ dlen,
                                                  const gm_verdict *__restrict__ verdicts, uint32_t n, JwtTab t,
                                                  uint4 *__restrict__ item0, uint4 *__restrict__ item1,
                                                  uint32_t *__restrict__ sig, uint32_t *__restrict__ ctl,
                                                  uint32_t *__restrict__ out_auth) {
    const uint64_t len = dlen ? min(*dlen, alen) : alen;
    for (uint32_t i0 = blockIdx.x * blockDim.x; i0 < n; i0 += gridDim.x * blockDim.x) {
        const uint32_t i = i0 + threadIdx.x;
        uint32_t nb = 0;
        if (i < n) {
            const uint4 v0 = reinterpret_cast<const uint4 *>(verdicts + i)[0];
            const uint4 v1 = reinterpret_cast<const uint4 *>(verdicts + i)[1];
            const uint32_t loc = v0.z, action = v1.x & 0xFF;
            uint32_t code = GM_AUTH_NONE;
            uint4 it0 = make_uint4(0, 0, 0, 0), it1 = it0;
            if ((action == GM_ACT_PROXY || action == GM_ACT_BLOCK) && loc != GM_NONE) {
                if (v0.x != t.gen || loc >= t.n_locs) code = jwt_code(GM_AUTH_DEFER, GM_AUTH_R_STALE);
                else if (t.auth && t.auth[loc].first_key != GM_NONE)
                    code = jwt_find(A, len, reqs + i, t, t.auth[loc], it0, it1, sig + 8 * (size_t)i);
            }
            if (code != GM_NONE) { out_auth[i] = code; it0.x = 0; }
            else item1[i] = it1;
            item0[i] = it0;
            nb = it0.x & JWT_NB_MASK;
        }
        jwt_bin_add(ctl + JWT_CTL_HIST, min(nb, JWT_BINS) - 1, nb != 0);
    }
}

__global__ __launch_bounds__(256) void k_jwt_order(const uint4 *__restrict__ item0, uint32_t n, uint32_t *__restrict__ ctl,
                                                   uint32_t *__restrict__ order) {
    __shared__ uint32_t base[JWT_BINS];
    if (threadIdx.x < JWT_BINS) {
        const uint32_t h = ctl[JWT_CTL_HIST + threadIdx.x];
        uint32_t inc = h;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(inc, d);
            if (threadIdx.x >= d) inc += u;
        }
        base[threadIdx.x] = inc - h;
        if (blockIdx.x == 0 && threadIdx.x == JWT_BINS - 1) ctl[0] = inc;
    }
    __syncthreads();
    for (uint32_t i0 = blockIdx.x * blockDim.x; i0 < n; i0 += gridDim.x * blockDim.x) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t nb = i < n ? item0[i].x & JWT_NB_MASK : 0u;
        const uint32_t bin = min(nb, JWT_BINS) - 1;
        const uint32_t pos = jwt_bin_add(ctl + JWT_CTL_CUR, bin, nb != 0);
        if (nb) order[min(base[bin & (JWT_BINS - 1)] + pos, n - 1)] = i;
    }
}

__device__ __forceinline__ uint32_t sha_ror(uint32_t x, uint32_t k) { return __builtin_amdgcn_alignbit(x, x, k); }
// one SHA-256 compress of the block w into H; w is consumed (the schedule rolls through it)
__device__ __forceinline__ void sha256_compress(uint32_t (&H)[8], uint32_t (&w)[16]) {
    uint32_t a = H[0], b = H[1], c = H[2], d = H[3], e = H[4], f = H[5], g = H[6], h = H[7];
#pragma unroll
    for (uint32_t i = 0; i < 64; i++) {
        if (i >= 16) {
            const uint32_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
            w[i & 15] += (sha_ror(x, 7) ^ sha_ror(x, 18) ^ (x >> 3)) + w[(i + 9) & 15] + (sha_ror(y, 17) ^ sha_ror(y, 19) ^ (y >> 10));
        }
        const uint32_t t1 = h + (sha_ror(e, 6) ^ sha_ror(e, 11) ^ sha_ror(e, 25)) + (g ^ (e & (f ^ g))) + sha256_k(i) + w[i & 15];
        const uint32_t t2 = (sha_ror(a, 2) ^ sha_ror(a, 13) ^ sha_ror(a, 22)) + ((a & b) | (c & (a | b)));
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    H[0] += a; H[1] += b; H[2] += c; H[3] += d; H[4] += e; H[5] += f; H[6] += g; H[7] += h;
}

__global__ __launch_bounds__(256) void k_jwt_hmac(const uint8_t *__restrict__ A, uint32_t *__restrict__ ctl,
                                                  const uint32_t *__restrict__ order, uint4 *__restrict__ item0,
                                                  const uint4 *__restrict__ item1, uint32_t *__restrict__ sig,
                                                  const DJwk *__restrict__ keys, uint32_t n, uint32_t *__restrict__ rlist,
                                                  uint32_t *__restrict__ out_auth) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= min(ctl[0], n)) return;
    const uint32_t i = min(order[gid], n - 1);
    const uint4 it0 = item0[i], it1 = item1[i];
    const uint32_t nb = it0.x & JWT_NB_MASK, len = it0.y;
    const bool rsa = it0.x & JWT_RSA;   // plain SHA-256 of the signing input: the digest is k_jwt_rsa's or k_jwt_ec's
    const uint32_t bits = ((rsa ? 0u : 64u) + len) * 8u;   // (an HMAC's key block came first)
    const uint64_t text = (uint64_t)it0.z | (uint64_t)it0.w << 32;
    const uint32_t s = (uint32_t)text & 3u, sel = 0x00010203u + 0x01010101u * s;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(A + (text - s));   // the dword that holds text byte 0
    const uint4 g0 = reinterpret_cast<const uint4 *>(sig + 8 * (size_t)i)[0], g1 = reinterpret_cast<const uint4 *>(sig + 8 * (size_t)i)[1];
    bool ok = false;
    for (uint32_t m = it1.y & ((1u << JWT_KEYS_MAX) - 1); m && !ok; m &= m - 1) {
        const DJwk *K = keys + it1.x + (uint32_t)__builtin_ctz(m);
        uint32_t H[8], w[16];
        {
            const uint4 p = reinterpret_cast<const uint4 *>(K->inner)[0], q = reinterpret_cast<const uint4 *>(K->inner)[1];
            H[0] = p.x; H[1] = p.y; H[2] = p.z; H[3] = p.w; H[4] = q.x; H[5] = q.y; H[6] = q.z; H[7] = q.w;
        }
        if (rsa) {
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) H[j] = SHA256_IV[j];
        }
        for (uint32_t b = 0; b < nb; b++) {
            const uint32_t *blk = src + 16 * b;
            const int rem = (int)len - (int)(64 * b);   // text bytes from this block on (<= 0: padding only)
            if (rem >= 64) {
                uint32_t d[17];
#pragma unroll
                for (uint32_t j = 0; j < 17; j++) d[j] = blk[j];
#pragma unroll
                for (uint32_t j = 0; j < 16; j++) w[j] = __builtin_amdgcn_perm(d[j + 1], d[j], sel);
            } else {
                const int have = rem + (int)s;   // dword j holds a text byte iff 4 j < have
                uint32_t d[17];
#pragma unroll
                for (int j = 0; j < 17; j++) d[j] = 4 * j < have ? blk[j] : 0u;
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    uint32_t x = __builtin_amdgcn_perm(d[j + 1], d[j], sel);
                    const int keep = rem - 4 * j;   // text bytes in this word
                    if (keep < 4) {
                        x = keep <= 0 ? 0u : x & ~(0xFFFFFFFFu >> (8 * keep));
                        if (keep >= 0) x |= 0x80000000u >> (8 * keep);
                    }
                    w[j] = x;
                }
                if (b + 1 == nb) { w[14] = 0; w[15] = bits; }
            }
            sha256_compress(H, w);
        }
        if (rsa) {
            reinterpret_cast<uint4 *>(sig + 8 * (size_t)i)[0] = make_uint4(H[0], H[1], H[2], H[3]);
            reinterpret_cast<uint4 *>(sig + 8 * (size_t)i)[1] = make_uint4(H[4], H[5], H[6], H[7]);
            break;
        }
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) w[j] = H[j];
        w[8] = 0x80000000u;
#pragma unroll
        for (uint32_t j = 9; j < 15; j++) w[j] = 0;
        w[15] = (64u + 32u) * 8u;
        {
            const uint4 p = reinterpret_cast<const uint4 *>(K->outer)[0], q = reinterpret_cast<const uint4 *>(K->outer)[1];
            H[0] = p.x; H[1] = p.y; H[2] = p.z; H[3] = p.w; H[4] = q.x; H[5] = q.y; H[6] = q.z; H[7] = q.w;
        }
        sha256_compress(H, w);
        const uint32_t diff = (H[0] ^ g0.x) | (H[1] ^ g0.y) | (H[2] ^ g0.z) | (H[3] ^ g0.w) |
                              (H[4] ^ g1.x) | (H[5] ^ g1.y) | (H[6] ^ g1.z) | (H[7] ^ g1.w);
        ok = diff == 0;
    }
    const uint32_t cls = it0.x >> JWT_CLS_SHIFT & 3u;
    const uint32_t pos = jwt_bin_add(ctl + JWT_CTL_RSA, cls, rsa);
    if (rsa) rlist[(size_t)cls * n + min(pos, n - 1)] = i;   // (class 3 only where the generation has an EC key: 4 n words)
    else if (ok) item0[i].x = nb | JWT_VERIFIED;
    else out_auth[i] = jwt_code(GM_AUTH_DENY, GM_AUTH_R_SIGNATURE);
}

// The K-limb integer s that segment 3 (S: jwt_rsa_chars(K) characters) begins with, least significant
// limb first, into the lane's LDS column a[64 j]; whether s < n.  Limb j is stream bits
// [32 (K - 1 - j), 32 (K - j)): at most seven characters, all of them the segment's.
template <uint32_t K>
__device__ bool jwt_rsa_sig(const uint8_t *S, const uint32_t *__restrict__ nn, uint32_t *a) {
    uint32_t bw = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < K; j++) {
        const uint32_t lo = 32 * (K - 1 - j), c1 = (lo + 31) / 6;
        unsigned long long acc = 0;
        for (uint32_t c = lo / 6; c <= c1; c++) acc = acc << 6 | jwt_b64v(S[c]);
        const uint32_t v = (uint32_t)(acc >> (6 * (c1 + 1) - (lo + 32)));
        a[64 * j] = v;
        bw = (uint32_t)(((uint64_t)v - nn[j] - bw) >> 63);
    }
    return bw != 0;
}

// limb j of the EMSA-PKCS1-v1_5 encoding of a SHA-256 digest (eight big-endian words d), K limbs in all
template <uint32_t K>
__device__ __forceinline__ uint32_t jwt_rsa_em(const uint32_t (&d)[8], uint32_t j) {
    constexpr uint32_t di[5] = {0x05000420u, 0x03040201u, 0x86480165u, 0x0D060960u, 0x00303130u};   // DigestInfo, 00 before it
    return j < 8 ? d[7 - j] : j < 13 ? di[j - 8] : j + 1 < K ? 0xFFFFFFFFu : 0x0001FFFFu;
}

template <uint32_t K, bool NREG>   // NREG: n in VGPRs as well (else four limbs a load, every row)
__global__ __launch_bounds__(64) void k_jwt_rsa(const uint8_t *__restrict__ A, const uint32_t *__restrict__ ctl,
                                                const uint32_t *__restrict__ rlist, uint32_t cls, uint4 *__restrict__ item0,
                                                const uint4 *__restrict__ item1, const uint32_t *__restrict__ dig, JwtTab t,
                                                uint32_t n, uint32_t *__restrict__ out_auth) {
    __shared__ uint32_t lds[K * 64];
    const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
    if (gid >= min(ctl[JWT_CTL_RSA + cls], n)) return;
    const uint32_t i = min(rlist[(size_t)cls * n + gid], n - 1);
    const uint4 it0 = item0[i], it1 = item1[i];
    const uint8_t *S = A + ((uint64_t)it0.z | (uint64_t)it0.w << 32) + it0.y + 1;   // segment 3
    uint32_t *a = lds + threadIdx.x;
    uint32_t d[8];
    {
        const uint4 p = reinterpret_cast<const uint4 *>(dig + 8 * (size_t)i)[0], q = reinterpret_cast<const uint4 *>(dig + 8 * (size_t)i)[1];
        d[0] = p.x; d[1] = p.y; d[2] = p.z; d[3] = p.w; d[4] = q.x; d[5] = q.y; d[6] = q.z; d[7] = q.w;
    }
    bool ok = false;
    for (uint32_t m = it1.y & ((1u << JWT_KEYS_MAX) - 1); m && !ok; m &= m - 1) {
        const DJwk *J = t.keys + it1.x + (uint32_t)__builtin_ctz(m);
        if (J->limbs != K) continue;
        const uint32_t *nn = t.limbs + J->limb_off;   // n[K], RR[K]: 16-byte aligned
        const uint4 *nq = reinterpret_cast<const uint4 *>(nn);
        const uint32_t n0 = J->inner[0];
        if (!jwt_rsa_sig<K>(S, nn, a)) continue;      // a = s, and s < n
        uint32_t b[K], tt[K + 1], nr[NREG ? K : 16];
#pragma unroll
        for (uint32_t j = 0; j < K; j += 4) {         // b = RR
            const uint4 v = nq[(K + j) / 4];
            b[j] = v.x; b[j + 1] = v.y; b[j + 2] = v.z; b[j + 3] = v.w;
            if (NREG) { const uint4 u = nq[j / 4]; nr[j] = u.x; nr[j + 1] = u.y; nr[j + 2] = u.z; nr[j + 3] = u.w; }
        }
        // n's limb j: from the registers, or from a ring of four loads (16 limbs) that runs three loads
        // ahead of the limb in use and on into the next row (K / 4 is a multiple of 4)
#define JWT_RSA_N(j) nr[NREG ? (j) : (j) & 15]
#define JWT_RSA_NLOAD(g) \
        { const uint4 u = nq[(g) % (K / 4)]; nr[(g) % 4 * 4] = u.x; nr[(g) % 4 * 4 + 1] = u.y; nr[(g) % 4 * 4 + 2] = u.z; nr[(g) % 4 * 4 + 3] = u.w; }
#pragma unroll 1
        for (uint32_t r = 0; r < 18; r++) {           // y = mont(a, b): s RR, sixteen squarings, y s
#pragma unroll
            for (uint32_t j = 0; j <= K; j++) tt[j] = 0;
            if (!NREG) { JWT_RSA_NLOAD(0) JWT_RSA_NLOAD(1) JWT_RSA_NLOAD(2) }
#pragma unroll 1
            for (uint32_t row = 0; row < K; row++) {
                const uint32_t ai = a[64 * row];
                uint32_t mq = 0;
                uint64_t x = 0, y = 0;
#pragma unroll
                for (uint32_t j = 0; j < K; j++) {
                    // the addends, carries folded in, are opaque to the compiler: each multiply-add then waits
                    // for its chain (left free, all K products a_i b[j] + t[j] are formed ahead: K more VGPRs),
                    // and at each fourth limb the load of the ring's next four is held to this place
                    uint64_t ax = (uint64_t)tt[j] + (uint32_t)(x >> 32);
                    if (!NREG && (j & 3) == 0) {
                        asm volatile("" : "+v"(ax) : : "memory");
                        JWT_RSA_NLOAD(j / 4 + 3)
                    } else asm("" : "+v"(ax));
                    x = (uint64_t)ai * b[j] + ax;
                    if (j == 0) mq = (uint32_t)x * n0;
                    uint64_t ay = (uint64_t)(uint32_t)x + (uint32_t)(y >> 32);
                    asm("" : "+v"(ay));
                    y = (uint64_t)mq * JWT_RSA_N(j) + ay;
                    if (j) tt[j - 1] = (uint32_t)y;   // (limb 0 is zero: that is what m was chosen for)
                }
                const uint64_t z = (uint64_t)tt[K] + (x >> 32) + (y >> 32);
                tt[K - 1] = (uint32_t)z; tt[K] = (uint32_t)(z >> 32);
            }
            // t < 2 n: subtract n once if t >= n (the borrow of t - n first, then the subtraction)
            if (!NREG) asm volatile("" ::: "memory");   // (n's loads below stay below the rows)
            uint32_t bw = 0;
#pragma unroll
            for (uint32_t j = 0; j < K; j++) bw = (uint32_t)(((uint64_t)tt[j] - (NREG ? nr[NREG ? j : 0] : nn[j]) - bw) >> 63);
            const uint32_t sub = (tt[K] | (bw ^ 1u)) ? 0xFFFFFFFFu : 0u;
            bw = 0;
#pragma unroll
            for (uint32_t j = 0; j < K; j++) {
                const uint64_t v = (uint64_t)tt[j] - ((NREG ? nr[NREG ? j : 0] : nn[j]) & sub) - bw;
                b[j] = (uint32_t)v;
                bw = (uint32_t)(v >> 63);
            }
            // the next multiplier: y, and s for the last product (b = y either way)
            if (r == 16) jwt_rsa_sig<K>(S, nn, a);
            else if (r < 16) {
#pragma unroll
                for (uint32_t j = 0; j < K; j++) a[64 * j] = b[j];
            }
        }
#undef JWT_RSA_N
#undef JWT_RSA_NLOAD
        uint32_t diff = 0;
#pragma unroll
        for (uint32_t j = 0; j < K; j++) diff |= b[j] ^ jwt_rsa_em<K>(d, j);
        ok = diff == 0;
    }
    if (ok) item0[i].x = it0.x | JWT_VERIFIED;
    else out_auth[i] = jwt_code(GM_AUTH_DENY, GM_AUTH_R_SIGNATURE);
}

// ES256's hot path: a lane per token of the fourth list, 64-thread groups.  The whole verification lives in the
// lane's VGPRs (gm_p256.hpp: ecdsa_verify) -- no LDS; the key's table is read through the key pointer, four
// dwordx4 loads a ladder step (the lanes of a wave nearly always share the key: at most 15 distinct 64-byte
// entries).  r | s are decoded from the token's own characters: limb j of the 512-bit integer is stream bits
// [32 (15 - j), 32 (16 - j)), at most seven characters, all of them the segment's 86.
__global__ __launch_bounds__(64) void k_jwt_ec(const uint8_t *__restrict__ A, const uint32_t *__restrict__ ctl,
                                               const uint32_t *__restrict__ rlist, uint4 *__restrict__ item0,
                                               const uint4 *__restrict__ item1, const uint32_t *__restrict__ dig, JwtTab t,
                                               uint32_t n, uint32_t *__restrict__ out_auth) {
    const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
    if (gid >= min(ctl[JWT_CTL_RSA + JWT_CLS_EC], n)) return;
    const uint32_t i = min(rlist[(size_t)JWT_CLS_EC * n + gid], n - 1);
    const uint4 it0 = item0[i], it1 = item1[i];
    const uint8_t *S = A + ((uint64_t)it0.z | (uint64_t)it0.w << 32) + it0.y + 1;   // segment 3
    p256::Fe e, r, s;
    {
        const uint4 p = reinterpret_cast<const uint4 *>(dig + 8 * (size_t)i)[0], q = reinterpret_cast<const uint4 *>(dig + 8 * (size_t)i)[1];
        e.v[7] = p.x; e.v[6] = p.y; e.v[5] = p.z; e.v[4] = p.w; e.v[3] = q.x; e.v[2] = q.y; e.v[1] = q.z; e.v[0] = q.w;
    }
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
        const uint32_t lo = 32 * (15 - j), c1 = (lo + 31) / 6;
        unsigned long long acc = 0;
#pragma unroll
        for (uint32_t c = lo / 6; c <= c1; c++) acc = acc << 6 | jwt_b64v(S[c]);
        const uint32_t v = (uint32_t)(acc >> (6 * (c1 + 1) - (lo + 32)));
        if (j < 8) s.v[j] = v; else r.v[j - 8] = v;
    }
    bool ok = false;
    for (uint32_t m = it1.y & ((1u << JWT_KEYS_MAX) - 1); m && !ok; m &= m - 1) {   // (only a lane that failed goes round again)
        const DJwk *J = t.keys + it1.x + (uint32_t)__builtin_ctz(m);   // (an EC key: k_jwt_find masked with ec_mask)
        ok = p256::ecdsa_verify(e, r, s, t.limbs + J->limb_off);
    }
    if (ok) item0[i].x = it0.x | JWT_VERIFIED;
    else out_auth[i] = jwt_code(GM_AUTH_DENY, GM_AUTH_R_SIGNATURE);
}

__global__ __launch_bounds__(256) void k_jwt_claims(const uint8_t *__restrict__ A, const uint32_t *__restrict__ ctl,
                                                    const uint32_t *__restrict__ order, const uint4 *__restrict__ item0,
                                                    const uint4 *__restrict__ item1, uint32_t n, long long now,
                                                    uint32_t *__restrict__ out_auth) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= min(ctl[0], n)) return;
    const uint32_t i = min(order[gid], n - 1);
    const uint4 it0 = item0[i];
    if (!(it0.x & JWT_VERIFIED)) return;
    const uint4 it1 = item1[i];
    const uint64_t text = (uint64_t)it0.z | (uint64_t)it0.w << 32;
    JwtRd rd;
    JwtDoc d;
    rd.init(A + text + it1.z, it0.y - it1.z);
    const JwtTab none{};
    const DAuth na{};
    uint32_t code = jwt_code(GM_AUTH_OK, 0);
    const long long leeway = (long long)it1.w;
    if (!jwt_walk(rd, false, none, na, d)) code = jwt_code(GM_AUTH_DENY, GM_AUTH_R_MALFORMED);
    else if (d.has_exp && !(d.exp + leeway > now)) code = jwt_code(GM_AUTH_DENY, GM_AUTH_R_EXPIRED);
    else if (d.has_nbf && !(d.nbf <= now + leeway)) code = jwt_code(GM_AUTH_DENY, GM_AUTH_R_NOT_YET);
    out_auth[i] = code;
}
