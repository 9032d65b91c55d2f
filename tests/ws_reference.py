"""gm_ws_messages' grammar (include/gpumatch.h, gm_ws.inc) restated as a plain serial Python loop:
what the kernel is compared with.

A segment is a run of one connection's client-to-server bytes that begins at a frame boundary with
no message open.  Frames (RFC 6455) are read left to right: byte 0 = FIN | RSV1-3 | opcode, byte 1 =
MASK | len7, len7 == 126 / 127 is followed by a 16 / 64-bit big-endian length, then the 4-byte key;
payload byte k is wire ^ key[k & 3].  The first two bytes are judged as soon as both are there, the
first reason of REASONS that applies wins; then RSV1 on a data frame stops with DEFLATE; then the
length form (LENGTH) once its bytes are there.  A frame that runs past the segment stops with OK.

parse(seg) -> (view, status, reason, consumed, stop, n_messages)."""

OK, CLOSED, DEFLATE, PROTO = 0, 1, 2, 3
REASONS = ["", "RSV", "OPCODE", "UNMASKED", "CTRL_FRAG", "CTRL_LEN", "LENGTH", "CONT", "NESTED"]
RSV, OPCODE, UNMASKED, CTRL_FRAG, CTRL_LEN, LENGTH, CONT, NESTED = range(1, 9)


def frame(opcode, payload=b"", fin=True, key=b"\x11\x22\x33\x44", rsv=0, masked=True, length_form=None):
    """One frame; rsv: RSV1 = 4, RSV2 = 2, RSV3 = 1; length_form 0 / 2 / 8 forces the 7 / 16 / 64-bit form."""
    n = len(payload)
    form = length_form if length_form is not None else (0 if n < 126 else 2 if n < 65536 else 8)
    b1 = (0x80 if masked else 0) | (n if form == 0 else 126 if form == 2 else 127)
    head = bytes([(0x80 if fin else 0) | rsv << 4 | opcode, b1]) + (n.to_bytes(form, "big") if form else b"")
    if not masked:
        return head + payload
    return head + key + bytes(c ^ key[k & 3] for k, c in enumerate(payload))


def parse(seg):
    n, p, consumed, n_messages = len(seg), 0, 0, 0
    view, msg, is_open = [], [], False
    while True:
        if n - p < 2:            # read out (p == n), or a header cut short
            return b"".join(view), OK, 0, consumed, p, n_messages
        b0, b1 = seg[p], seg[p + 1]
        fin, rsv, op, masked, len7 = b0 >> 7, b0 >> 4 & 7, b0 & 15, b1 >> 7, b1 & 127
        ctrl, reason = op >= 8, 0
        if rsv & 3 or (rsv & 4 and (ctrl or op == 0)):
            reason = RSV
        elif 3 <= op <= 7 or op >= 0xB:
            reason = OPCODE
        elif not masked:
            reason = UNMASKED
        elif ctrl and not fin:
            reason = CTRL_FRAG
        elif ctrl and len7 > 125:
            reason = CTRL_LEN
        elif op == 0 and not is_open:
            reason = CONT
        elif op in (1, 2) and is_open:
            reason = NESTED
        if reason:
            return b"".join(view), PROTO, reason, consumed, p, n_messages
        if rsv & 4:
            return b"".join(view), DEFLATE, 0, consumed, p, n_messages
        ext = 2 if len7 == 126 else 8 if len7 == 127 else 0
        if n - p < 2 + ext:
            return b"".join(view), OK, 0, consumed, p, n_messages
        plen = int.from_bytes(seg[p + 2:p + 2 + ext], "big") if ext else len7
        if (ext == 2 and plen < 126) or (ext == 8 and (plen < 65536 or plen >> 63)):
            return b"".join(view), PROTO, LENGTH, consumed, p, n_messages
        ps = p + 2 + ext + 4
        if ps + plen > n:
            return b"".join(view), OK, 0, consumed, p, n_messages
        key = seg[ps - 4:ps]
        if op == 8:
            return b"".join(view), CLOSED, 0, ps + plen, p, n_messages
        if not ctrl:
            msg.append(bytes(c ^ key[k & 3] for k, c in enumerate(seg[ps:ps + plen])))
            is_open = not fin
            if fin:
                view += msg + [b"\n"]
                msg, n_messages = [], n_messages + 1
        p = ps + plen
        if not is_open:
            consumed = p
