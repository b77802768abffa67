"""TEST INFRASTRUCTURE ONLY: a plain-Python restatement of the reference's send-side header chain, written from its
behaviour (as oracle/ restates the receive side), for the dk_tx_serialize tests to compare against bit for bit.

    TcpHeader::serialize_and_attach   src/rust/inetstack/protocols/layer4/tcp/header.rs:330-405
      TcpOptions2::serialize :56-101, compute_size :43-54 / :408-421, tcp_checksum :433-509
    UdpHeader::serialize_and_attach   layer4/udp/header.rs:97-130, checksum :140-193
    Ipv4Header::serialize_and_attach  layer3/ipv4/header.rs:229-266, Ipv4Header::new :88-104, compute_checksum :280-301
    Ethernet2Header::serialize_and_attach  layer2/ethernet2/header.rs:68-73

`serialize_batch` adds dk_tx_serialize's batch contract (include/dk_rx.h): the descriptor packing, the per-frame
statuses in their order, and headers written into the headroom in front of each payload.
tests/test_tx_serialize_abi.py pins this module against tests/frames.py's independent builders and the receive oracle.
"""
from __future__ import annotations

import struct

import numpy as np

OK, E_PROTO, E_OPTS, E_LINK, E_LEN, E_RANGE = range(6)
OFFLOAD_TCP, OFFLOAD_UDP = 1, 2
KIND_EOL, KIND_NOP, KIND_MSS, KIND_WS, KIND_SACK_OK, KIND_SACK, KIND_TS = 0, 1, 2, 3, 4, 5, 8


def fold(words_sum: int) -> int:
    """state = 0xffff + sum; while state > 0xffff: state -= 0xffff; !state (the reference's three checksum tails)."""
    state = 0xFFFF + words_sum
    while state > 0xFFFF:
        state -= 0xFFFF
    return (~state) & 0xFFFF


def be_words(data: bytes) -> int:
    """Sum of big-endian 16-bit words, an odd last byte padded with zero."""
    if len(data) % 2:
        data = data + b"\0"
    return int(np.frombuffer(data, ">u2").sum(dtype=np.uint64)) if data else 0


def option_entry(rec, k: int):
    """TcpOptions2::serialize of entry k of a dk_tcp_opts record -> bytes, or None if it has no serialized form."""
    e = rec["opt"][k]
    kind = int(e["kind"])
    if kind == KIND_EOL:
        return b""
    if kind == KIND_NOP:
        return b"\x01"
    if kind == KIND_MSS:
        return bytes([2, 4]) + struct.pack("!H", int(e["u16"]))
    if kind == KIND_WS:
        return bytes([3, 3, int(e["u8"])])
    if kind == KIND_SACK_OK:
        return bytes([4, 2])
    if kind == KIND_SACK:
        ns, first = int(e["u8"]), int(e["u16"])
        if not 1 <= ns <= 4 or first + ns > 4:
            return None
        out = bytes([5, 2 + 8 * ns])
        for s in range(ns):
            out += struct.pack("!II", int(rec["sack"][first + s][0]), int(rec["sack"][first + s][1]))
        return out
    if kind == KIND_TS:
        return bytes([8, 10]) + struct.pack("!II", int(e["v0"]), int(e["v1"]))
    return None


def tcp_option_bytes(rec):
    """The option area of a TCP header for one dk_tcp_opts record (None: no options): the entries, one EndOfOptionsList
    byte if the list is not empty, zero padding to a multiple of 4. None if the list cannot be serialized (more than 5
    entries, an entry without a form, a header over 60 bytes)."""
    if rec is None or int(rec["num"]) == 0:
        return b""
    if int(rec["num"]) > 5:
        return None
    out = b""
    for k in range(int(rec["num"])):
        b = option_entry(rec, k)
        if b is None:
            return None
        out += b
    out += b"\0"
    out += b"\0" * (-len(out) % 4)
    return out if 20 + len(out) <= 60 else None


def header_bytes(proto: int, rec=None) -> int:
    """dk_tx_header_bytes."""
    if proto == 17:
        return 42
    if proto != 6:
        return 0
    o = tcp_option_bytes(rec)
    return 0 if o is None else 54 + len(o)


def pseudo_sum(src_ip: int, dst_ip: int, proto: int, seglen: int) -> int:
    return be_words(int(src_ip).to_bytes(4, "little") + int(dst_ip).to_bytes(4, "little")) + proto + seglen


def tcp_header(payload: bytes, src_ip, dst_ip, sport, dport, seq, ack, ns, b13, window, urg, options: bytes,
               offload: bool) -> bytes:
    hl = 20 + len(options)
    h = bytearray(struct.pack("!HHIIBBHHH", sport, dport, seq, ack, ((hl // 4) << 4) | (1 if ns else 0), b13, window, 0,
                              urg)) + options
    if not offload:
        c = fold(pseudo_sum(src_ip, dst_ip, 6, hl + len(payload)) + be_words(bytes(h)) + be_words(payload))
        h[16:18] = struct.pack("!H", c)
    return bytes(h)


def udp_header(payload: bytes, src_ip, dst_ip, sport, dport, offload: bool) -> bytes:
    L = 8 + len(payload)
    h = bytearray(struct.pack("!HHHH", sport, dport, L & 0xFFFF, 0))
    if not offload:
        c = fold(pseudo_sum(src_ip, dst_ip, 17, L) + be_words(bytes(h)) + be_words(payload))
        h[6:8] = struct.pack("!H", c)
    return bytes(h)


def ipv4_header(total_length: int, proto: int, src_ip: int, dst_ip: int, ident=0, ttl=255, tos=0) -> bytes:
    h = bytearray(20)
    h[0] = 0x45
    h[1] = tos
    h[2:4] = struct.pack("!H", total_length)
    h[4:6] = struct.pack("!H", ident)
    h[6:8] = struct.pack("!H", 0x2 << 13)  # IPV4_CTRL_FLAG_DF, fragment offset 0
    h[8] = ttl
    h[9] = proto
    h[12:16] = int(src_ip).to_bytes(4, "little")
    h[16:20] = int(dst_ip).to_bytes(4, "little")
    w = struct.unpack("!10H", bytes(h))
    h[10:12] = struct.pack("!H", fold(sum(w) - w[5]))
    return bytes(h)


def headers(payload: bytes, proto: int, src_ip: int, dst_ip: int, ports: int, *, meta: int = 0, seq=0, ack=0, winurg=0,
            options: bytes = b"", ipw: int = 0x00FF0000, dst_mac=bytes(6), src_mac=bytes(6), flags: int = 0) -> bytes:
    """Ethernet2 + IPv4 + TCP / UDP header bytes of one segment, from dk_tx_segs-packed fields."""
    sport, dport = ports & 0xFFFF, ports >> 16
    if proto == 6:
        l4 = tcp_header(payload, src_ip, dst_ip, sport, dport, seq, ack, (meta >> 24) & 1, (meta >> 16) & 0xFF,
                        winurg & 0xFFFF, winurg >> 16, options, bool(flags & OFFLOAD_TCP))
    else:
        l4 = udp_header(payload, src_ip, dst_ip, sport, dport, bool(flags & OFFLOAD_UDP))
    ip = ipv4_header(20 + len(l4) + len(payload), proto, src_ip, dst_ip, ipw & 0xFFFF, (ipw >> 16) & 0xFF, ipw >> 24)
    return bytes(dst_mac) + bytes(src_mac) + b"\x08\x00" + ip + l4


def serialize_batch(blob: np.ndarray, segs: dict, links: np.ndarray, flags: int = 0, frames_bytes=None):
    """dk_tx_serialize over host arrays. segs: payload_off, payload_len, meta, src_ip, dst_ip, ports and optionally
    tcp_seq, tcp_ack, tcp_win, tcp_opts (TCP_OPTS_DTYPE), ip_word, link. links: records with dst_mac / src_mac.
    Returns (blob copy with the headers written, off_out u32, len_out u16, status u32)."""
    out = np.array(blob, np.uint8, copy=True)
    fb = out.size if frames_bytes is None else frames_bytes
    n = len(segs["payload_off"])
    off_out, len_out, status = np.zeros(n, np.uint32), np.zeros(n, np.uint16), np.zeros(n, np.uint32)
    get = lambda k, i, d=0: int(segs[k][i]) if segs.get(k) is not None else d  # noqa: E731
    for i in range(n):
        poff, plen, meta = int(segs["payload_off"][i]), int(segs["payload_len"][i]), int(segs["meta"][i])
        proto = (meta >> 8) & 0xFF
        if proto not in (6, 17):
            status[i] = E_PROTO
            continue
        options = b""
        if proto == 6:
            nib = meta >> 28
            if nib > 5:
                options = tcp_option_bytes(segs["tcp_opts"][i]) if segs.get("tcp_opts") is not None else None
                if options is None or 20 + len(options) != nib * 4:
                    status[i] = E_OPTS
                    continue
            elif nib not in (0, 5):
                status[i] = E_OPTS
                continue
        H = 42 if proto == 17 else 54 + len(options)
        link = get("link", i)
        if link >= len(links):
            status[i] = E_LINK
        elif H + plen > 65535:
            status[i] = E_LEN
        elif poff < H or poff + plen > fb:
            status[i] = E_RANGE
        if status[i]:
            continue
        payload = blob[poff:poff + plen].tobytes()
        h = headers(payload, proto, int(segs["src_ip"][i]), int(segs["dst_ip"][i]), int(segs["ports"][i]), meta=meta,
                    seq=get("tcp_seq", i), ack=get("tcp_ack", i), winurg=get("tcp_win", i), options=options,
                    ipw=get("ip_word", i, 0x00FF0000), dst_mac=bytes(links["dst_mac"][link]),
                    src_mac=bytes(links["src_mac"][link]), flags=flags)
        assert len(h) == H
        out[poff - H:poff] = np.frombuffer(h, np.uint8)
        off_out[i], len_out[i] = poff - H, H + plen
    return out, off_out, len_out, status


# ---------------------------------------------------------------------------------------------------------------------
# Builders shared by the CPU and GPU tests.
# ---------------------------------------------------------------------------------------------------------------------
def opts_record(entries):
    """A dk_tcp_opts record (TCP_OPTS_DTYPE scalar array of shape (1,)) from a list of ("mss", v), ("ws", v),
    ("sack_ok",), ("sack", [(begin, end), ...]), ("ts", sender, echo), ("nop",), ("eol",), ("raw", kind)."""
    from demikernel_amd._native import TCP_OPTS_DTYPE

    r = np.zeros(1, TCP_OPTS_DTYPE)
    r["num"] = len(entries)
    nsack = 0
    for k, e in enumerate(entries[:5]):
        o = r["opt"][0, k]
        if e[0] == "mss":
            o["kind"], o["u16"] = KIND_MSS, e[1]
        elif e[0] == "ws":
            o["kind"], o["u8"] = KIND_WS, e[1]
        elif e[0] == "sack_ok":
            o["kind"] = KIND_SACK_OK
        elif e[0] == "sack":
            o["kind"], o["u8"], o["u16"] = KIND_SACK, len(e[1]), nsack
            for b, en in e[1][:4 - nsack]:
                r["sack"][0, nsack] = (b, en)
                nsack += 1
        elif e[0] == "ts":
            o["kind"], o["v0"], o["v1"] = KIND_TS, e[1], e[2]
        elif e[0] == "nop":
            o["kind"] = KIND_NOP
        elif e[0] == "eol":
            o["kind"] = KIND_EOL
        else:
            o["kind"] = e[1]
    return r


SACK4 = [(0x01020304, 0x11121314), (0xFFFFFFFF, 0), (0x80000000, 0x7FFFFFFF), (5, 6)]


def option_cases():
    """(name, entries, hand-encoded option bytes before the EndOfOptionsList byte and the padding)."""
    ts = bytes([8, 10]) + struct.pack("!II", 0xDEADBEEF, 0x01020304)
    sack = lambda blocks: bytes([5, 2 + 8 * len(blocks)]) + b"".join(struct.pack("!II", b, e) for b, e in blocks)  # noqa: E731
    return [
        ("mss", [("mss", 1460)], bytes([2, 4, 0x05, 0xB4])),
        ("ws", [("ws", 7)], bytes([3, 3, 7])),
        ("sack_ok", [("sack_ok",)], bytes([4, 2])),
        ("ts", [("ts", 0xDEADBEEF, 0x01020304)], ts),
        ("nop", [("nop",)], bytes([1])),
        ("eol", [("eol",)], b""),
        ("sack1", [("sack", SACK4[:1])], sack(SACK4[:1])),
        ("sack4", [("sack", SACK4)], sack(SACK4)),
        ("mss_ws", [("mss", 536), ("ws", 14)], bytes([2, 4, 0x02, 0x18, 3, 3, 14])),  # active_open.rs:239-242's SYN
        ("nop_nop_ts", [("nop",), ("nop",), ("ts", 0xDEADBEEF, 0x01020304)], bytes([1, 1]) + ts),
        ("five", [("mss", 9000), ("ws", 0), ("sack_ok",), ("ts", 0xDEADBEEF, 0x01020304), ("nop",)],
         bytes([2, 4, 0x23, 0x28, 3, 3, 0, 4, 2]) + ts + bytes([1])),
        ("fill40", [("sack", SACK4[:3]), ("ts", 0xDEADBEEF, 0x01020304), ("nop",), ("nop",), ("nop",)],
         sack(SACK4[:3]) + ts + bytes([1, 1, 1])),
        ("two_sacks", [("sack", SACK4[:1]), ("sack", SACK4[1:3])], sack(SACK4[:1]) + sack(SACK4[1:3])),
    ]


def bad_option_cases():
    """(name, record) of lists with no serialized form."""
    six = opts_record([("nop",)] * 5)
    six["num"] = 6
    sack0 = opts_record([("sack", SACK4[:1])])
    sack0["opt"][0, 0]["u8"] = 0
    sack5 = opts_record([("sack", SACK4)])
    sack5["opt"][0, 0]["u8"] = 5
    return [
        ("num6", six),
        ("unknown_kind", opts_record([("raw", 9)])),
        ("sack0", sack0),
        ("sack5", sack5),
        ("over40", opts_record([("sack", SACK4), ("ts", 1, 2)])),  # 34 + 10 + EOL = 45 option bytes
    ]
