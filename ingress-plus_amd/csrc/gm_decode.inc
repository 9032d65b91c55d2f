// gm_decode.inc -- request parsers before the WAF stages (SURVEY.md §8 f4: Wallarm's
// parser_disable decoders), included into gm_device.hip's anonymous namespace.
//
// A signature set may declare the request parsers its rules are written against ("@decoders"
// in the GM_ENTRY_SIGS text); `wallarm_parser_disable <name>` (annotations.go:320-329 ->
// nginx.ingress.tmpl:26 server / :111 location) turns one off.  For every request whose location
// scans (waf_active) and runs a parser, gm_match_batch builds a SHADOW record -- same request
// index, $args and body replaced by their decoded views -- and runs the WAF stages a second time
// over the shadow arena; hits merge into the request's (one dedupe set).  The views, each part
// followed by '\n':
//   $args:  [the percent / urlenc transform of $args, if it changes a byte]
//           [each base64 run of $args, decoded]
//   body:   [the urlenc / percent transform of an application/x-www-form-urlencoded body, or the
//            JSON unescape of a body whose Content-Type contains "json", if it changes a byte]
//           [each base64 run of the body, decoded]
//   percent: %XX (two hex digits) -> the byte;  urlenc: '+' -> ' ' (with percent: both)
//   json_doc: \" \\ \/ \b \f \n \r \t and \uXXXX (surrogate pairs joined, a lone surrogate ->
//             U+FFFD) -> UTF-8; any other backslash pair stays as is
//   base64: a maximal run of >= 16 characters of [A-Za-z0-9+/]; its first 4 * floor(len / 4)
//           characters decoded (padding and a partial quantum ignored)
//   gzip: a body that is a gzip member, inflated to P (gm_inflate.inc, run before these passes);
//         after the body's parts above: [P] [the form / JSON transform of P by the body's kind, if
//         it changes a byte] [each base64 run of P, decoded]
//   multipart: a multipart/form-data body's part view M (gm_multipart.inc, run before these passes:
//         names, filenames and the contents under their transfer encodings); after everything
//         above: [M] [the JSON unescape of M if a part is JSON and it changes a byte] [each base64
//         run of M, decoded]
//   xml: an XML body's character-data view X (gm_xml.inc, run before these passes: text, quoted
//         attribute values and CDATA sections, references replaced, comments removed); after
//         everything above: [X] [each base64 run of X, decoded]
// One lane per request (byte loops over $args and the body); two passes around an exclusive scan.

constexpr uint32_t B64_MIN_RUN = 16;

__device__ __forceinline__ int dec_hexv(uint32_t c) {
    if (c - '0' < 10u) return (int)(c - '0');
    c |= 0x20;
    return c - 'a' < 6u ? (int)(c - 'a' + 10) : -1;
}

__device__ __forceinline__ int b64v(uint32_t c) {
    if (c - 'A' < 26u) return (int)(c - 'A');
    if (c - 'a' < 26u) return (int)(c - 'a' + 26);
    if (c - '0' < 10u) return (int)(c - '0' + 52);
    if (c == '+') return 62;
    if (c == '/') return 63;
    return -1;
}

// percent / urlenc transform of s[0, n) -> d (nullptr: length only); *chg = a byte changed
__device__ uint32_t dec_form(const uint8_t *s, uint32_t n, uint32_t mask, uint8_t *d, bool &chg) {
    const bool pct = mask & DEC_PERCENT, plus = mask & DEC_URLENC;
    uint32_t o = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t c = s[i];
        if (pct && c == '%' && i + 2 < n) {
            const int h = dec_hexv(s[i + 1]), l = dec_hexv(s[i + 2]);
            if (h >= 0 && l >= 0) { c = (uint32_t)(h << 4 | l); i += 2; chg = true; }
        } else if (plus && c == '+') { c = ' '; chg = true; }
        if (d) d[o] = (uint8_t)c;
        o++;
    }
    return o;
}

__device__ __forceinline__ uint32_t utf8_put(uint8_t *d, uint32_t o, uint32_t cp) {
    if (cp < 0x80) { if (d) d[o] = (uint8_t)cp; return 1; }
    if (cp < 0x800) { if (d) { d[o] = (uint8_t)(0xC0 | cp >> 6); d[o + 1] = (uint8_t)(0x80 | (cp & 63)); } return 2; }
    if (cp < 0x10000) {
        if (d) { d[o] = (uint8_t)(0xE0 | cp >> 12); d[o + 1] = (uint8_t)(0x80 | (cp >> 6 & 63)); d[o + 2] = (uint8_t)(0x80 | (cp & 63)); }
        return 3;
    }
    if (d) {
        d[o] = (uint8_t)(0xF0 | cp >> 18); d[o + 1] = (uint8_t)(0x80 | (cp >> 12 & 63));
        d[o + 2] = (uint8_t)(0x80 | (cp >> 6 & 63)); d[o + 3] = (uint8_t)(0x80 | (cp & 63));
    }
    return 4;
}

__device__ __forceinline__ int hex4(const uint8_t *s, uint32_t i, uint32_t n) {
    if (i + 4 > n) return -1;
    int v = 0;
    for (uint32_t k = 0; k < 4; k++) {
        const int h = dec_hexv(s[i + k]);
        if (h < 0) return -1;
        v = v << 4 | h;
    }
    return v;
}

// JSON string-escape decoding of s[0, n)
__device__ uint32_t dec_json(const uint8_t *s, uint32_t n, uint8_t *d, bool &chg) {
    uint32_t o = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t c = s[i];
        if (c != '\\' || i + 1 >= n) { if (d) d[o] = (uint8_t)c; o++; continue; }
        const uint32_t e = s[i + 1];
        uint32_t r = 0xFFFFFFFFu;
        switch (e) {
        case '"': r = '"'; break;
        case '\\': r = '\\'; break;
        case '/': r = '/'; break;
        case 'b': r = 8; break;
        case 'f': r = 12; break;
        case 'n': r = 10; break;
        case 'r': r = 13; break;
        case 't': r = 9; break;
        default: break;
        }
        if (r != 0xFFFFFFFFu) { if (d) d[o] = (uint8_t)r; o++; i++; chg = true; continue; }
        if (e == 'u') {
            int cp = hex4(s, i + 2, n);
            if (cp >= 0) {
                uint32_t adv = 5;
                if (cp >= 0xD800 && cp <= 0xDBFF) {
                    const int lo = (i + 7 < n && s[i + 6] == '\\' && s[i + 7] == 'u') ? hex4(s, i + 8, n) : -1;
                    if (lo >= 0xDC00 && lo <= 0xDFFF) { cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00); adv = 11; }
                    else cp = 0xFFFD;
                } else if (cp >= 0xDC00 && cp <= 0xDFFF) cp = 0xFFFD;
                o += utf8_put(d, o, (uint32_t)cp);
                i += adv;
                chg = true;
                continue;
            }
        }
        if (d) d[o] = (uint8_t)c;   // an unknown escape stays: the backslash, then its character
        o++;
    }
    return o;
}

// every base64 run of s[0, n), decoded, each followed by '\n'
__device__ uint32_t dec_b64(const uint8_t *s, uint32_t n, uint8_t *d) {
    uint32_t o = 0, i = 0;
    while (i < n) {
        if (b64v(s[i]) < 0) { i++; continue; }
        uint32_t j = i;
        while (j < n && b64v(s[j]) >= 0) j++;
        const uint32_t L = j - i;
        if (L >= B64_MIN_RUN) {
            for (uint32_t q = i; q + 4 <= i + (L & ~3u); q += 4) {
                const uint32_t v = (uint32_t)b64v(s[q]) << 18 | (uint32_t)b64v(s[q + 1]) << 12 |
                                   (uint32_t)b64v(s[q + 2]) << 6 | (uint32_t)b64v(s[q + 3]);
                if (d) { d[o] = (uint8_t)(v >> 16); d[o + 1] = (uint8_t)(v >> 8); d[o + 2] = (uint8_t)v; }
                o += 3;
            }
            if (d) d[o] = '\n';
            o++;
        }
        i = j;
    }
    return o;
}

// the body's kind from the first Content-Type line: 1 form, 2 json, 0 other
__device__ uint32_t body_kind(const uint8_t *A, const Rec &r, uint64_t hdrs) {
    HdrIt it{hdrs, hdrs + r.hdr_len};
    uint64_t ns, vs; uint32_t nl, vl;
    const uint8_t ct[13] = "content_type";
    while (hdr_next(A, it, ns, nl, vs, vl)) {
        if (!hdr_name_is(A, ns, nl, ct, 12)) continue;
        const char *form = "application/x-www-form-urlencoded";
        bool f = vl >= 33;
        for (uint32_t k = 0; f && k < 33; k++) f = lc(A[vs + k]) == (uint32_t)(uint8_t)form[k];
        if (f) return 1;
        for (uint32_t k = 0; k + 4 <= vl; k++)
            if (lc(A[vs + k]) == 'j' && lc(A[vs + k + 1]) == 's' && lc(A[vs + k + 2]) == 'o' && lc(A[vs + k + 3]) == 'n')
                return 2;
        return 0;
    }
    return 0;
}

// the body's transform by its kind, then its base64 runs, of s[0, n) -> db + b (nullptr: sizes)
__device__ uint32_t dec_body(const uint8_t *s, uint32_t n, uint32_t kind, uint32_t mask, uint8_t *db, uint32_t b) {
    if (kind == 1 && (mask & (DEC_PERCENT | DEC_URLENC))) {
        bool chg = false;
        const uint32_t k = dec_form(s, n, mask, nullptr, chg);
        if (chg) {
            if (db) { dec_form(s, n, mask, db + b, chg); db[b + k] = '\n'; }
            b += k + 1;
        }
    } else if (kind == 2 && (mask & DEC_JSON)) {
        bool chg = false;
        const uint32_t k = dec_json(s, n, nullptr, chg);
        if (chg) {
            if (db) { dec_json(s, n, db + b, chg); db[b + k] = '\n'; }
            b += k + 1;
        }
    }
    if (mask & DEC_BASE64) b += dec_b64(s, n, db ? db + b : nullptr);
    return b;
}

// shadow record of request i: sizes (d = nullptr) or bytes at d; returns {args', body'} lengths.
// P[0, pn): the body inflated (pn = GM_NONE: none); M[0, mn): its multipart view, mflags its flags;
// X[0, xn): its xml view
__device__ uint2 dec_one(const uint8_t *A, const Rec &r, uint32_t mask, uint8_t *d, const uint8_t *P = nullptr,
                         uint32_t pn = GM_NONE, const uint8_t *M = nullptr, uint32_t mn = GM_NONE, uint32_t mflags = 0,
                         const uint8_t *X = nullptr, uint32_t xn = GM_NONE) {
    const uint64_t args = r.base + r.uri_len, hdrs = args + r.args_len, body = hdrs + r.hdr_len;
    uint32_t a = 0, b = 0;
    if (mask & (DEC_PERCENT | DEC_URLENC)) {
        bool chg = false;
        const uint32_t k = dec_form(A + args, r.args_len, mask, nullptr, chg);
        if (chg) {
            if (d) dec_form(A + args, r.args_len, mask, d, chg);
            if (d) d[k] = '\n';
            a += k + 1;
        }
    }
    if (mask & DEC_BASE64) a += dec_b64(A + args, r.args_len, d ? d + a : nullptr);
    uint8_t *db = d ? d + a : nullptr;
    const uint32_t kind = (mask & (DEC_PERCENT | DEC_URLENC | DEC_JSON)) ? body_kind(A, r, hdrs) : 0u;
    b = dec_body(A + body, r.body_len, kind, mask, db, b);
    if (pn != GM_NONE) {
        if (db) { for (uint32_t k = 0; k < pn; k++) db[b + k] = P[k]; db[b + pn] = '\n'; }
        b = dec_body(P, pn, kind, mask, db, b + pn + 1);
    }
    if (mn != GM_NONE) {
        if (db) { for (uint32_t k = 0; k < mn; k++) db[b + k] = M[k]; db[b + mn] = '\n'; }
        b = dec_body(M, mn, (mflags & 1) ? 2u : 0u, mask, db, b + mn + 1);
    }
    if (xn != GM_NONE) {
        if (db) { for (uint32_t k = 0; k < xn; k++) db[b + k] = X[k]; db[b + xn] = '\n'; }
        b = dec_body(X, xn, 0u, mask, db, b + xn + 1);
    }
    return make_uint2(a, b);
}

__device__ __forceinline__ uint32_t dec_mask_of(const gm_verdict &v, const GTab &t) {
    if (!waf_active(v) || v.location_id >= t.n_locs) return 0;
    return (t.loc_uri[v.location_id].flags >> LOCURI_DEC_SHIFT) & 127u;
}

__global__ void k_dec_size(const gm_req *__restrict__ reqs, const uint8_t *__restrict__ A, uint32_t n, GTab t,
                           const gm_verdict *__restrict__ out, uint64_t *__restrict__ sizes,
                           const uint8_t *__restrict__ Z, const uint64_t *__restrict__ zoff,
                           const uint32_t *__restrict__ zlen, const uint8_t *__restrict__ MV,
                           const uint64_t *__restrict__ moff, const uint32_t *__restrict__ mlen,
                           const uint32_t *__restrict__ mflg, const uint8_t *__restrict__ XV,
                           const uint64_t *__restrict__ xoff, const uint32_t *__restrict__ xlen) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t mask = dec_mask_of(out[i], t);
        uint64_t sz = 0;
        if (mask) {
            const bool gz = Z && (mask & DEC_GZIP);
            const bool mp = MV && (mask & DEC_MULTIPART);
            const bool xm = XV && (mask & DEC_XML);
            const uint2 ab = dec_one(A, load_rec(reqs + i), mask, nullptr, gz ? Z + zoff[i] : nullptr, gz ? zlen[i] : GM_NONE,
                                     mp ? MV + moff[i] : nullptr, mp ? mlen[i] : GM_NONE, mp ? mflg[i] : 0u,
                                     xm ? XV + xoff[i] : nullptr, xm ? xlen[i] : GM_NONE);
            sz = ((uint64_t)ab.x + ab.y + 15) & ~15ull;
        }
        sizes[i] = sz;
        if (i + 1 == n) sizes[n] = 0;
    }
}

// shadow records + bytes; blk2rec of the shadow arena (as k_route's); *len_dev = the arena length
__global__ void k_dec_emit(const gm_req *__restrict__ reqs, const uint8_t *__restrict__ A, uint32_t n, GTab t,
                           const gm_verdict *__restrict__ out, const uint64_t *__restrict__ base,
                           gm_req *__restrict__ sreqs, uint8_t *__restrict__ SA, uint64_t cap,
                           uint32_t *__restrict__ blk2rec, uint32_t nblk, uint64_t *__restrict__ len_dev,
                           uint32_t *__restrict__ status, const uint8_t *__restrict__ Z,
                           const uint64_t *__restrict__ zoff, const uint32_t *__restrict__ zlen,
                           const uint8_t *__restrict__ MV, const uint64_t *__restrict__ moff,
                           const uint32_t *__restrict__ mlen, const uint32_t *__restrict__ mflg,
                           const uint8_t *__restrict__ XV, const uint64_t *__restrict__ xoff,
                           const uint32_t *__restrict__ xlen) {
    const uint64_t total = base[n];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *len_dev = min(total, cap);
        if (total > cap) atomicOr(status + 3, 64u);
    }
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint64_t b = base[i];
        const uint64_t sz = base[i + 1] - b;
        gm_req s = {};
        s.base = min(b, cap & ~15ull);
        const uint32_t mask = dec_mask_of(out[i], t);
        if (mask && sz && b + sz <= cap) {
            const Rec r = load_rec(reqs + i);
            const bool gz = Z && (mask & DEC_GZIP);
            const bool mp = MV && (mask & DEC_MULTIPART);
            const bool xm = XV && (mask & DEC_XML);
            const uint2 ab = dec_one(A, r, mask, SA + b, gz ? Z + zoff[i] : nullptr, gz ? zlen[i] : GM_NONE,
                                     mp ? MV + moff[i] : nullptr, mp ? mlen[i] : GM_NONE, mp ? mflg[i] : 0u,
                                     xm ? XV + xoff[i] : nullptr, xm ? xlen[i] : GM_NONE);
            s.args_len = ab.x; s.body_len = ab.y;
            for (uint64_t k = b + ab.x + ab.y; k < b + sz; k++) SA[k] = 0;   // the slot's alignment tail
        }
        sreqs[i] = s;
        // blocks whose start lies in [base_i, base_{i+1}) belong to shadow record i
        const uint64_t b0 = i == 0 ? 0 : s.base;
        const uint64_t b1 = i + 1 < n ? min(base[i + 1], cap & ~15ull) : cap;
        uint64_t k0 = (b0 + (1u << BLK_SHIFT) - 1) >> BLK_SHIFT, k1 = (b1 + (1u << BLK_SHIFT) - 1) >> BLK_SHIFT;
        if (i + 1 == n) k1 = nblk;
        for (uint64_t k = k0; k < k1 && k < nblk; k++) blk2rec[k] = i;
    }
}
