"""Case builder for the active-open tests: a client (Bob) with connecting sockets, the servers that answer them, and the
batches the tests need. Frames are real Ethernet / IPv4 / TCP bytes (tests/frames.py); the receive results the model and
the device consume come from the receive oracle (CPU tests) or the receive engine (GPU tests) over the same bytes."""
from __future__ import annotations

import numpy as np

import frames as F
import tcp_connect_reference as R
import tcp_listen_cases as LC
from demikernel_amd import SocketId, flow_array, ipv4, ipv4_str
from demikernel_amd import tcp_connect as TC

FIN, SYN, RST, PSH, ACK = R.FIN, R.SYN, R.RST, R.PSH, R.ACK
BOB, BOB_IP, LINKS, NOW = LC.BOB, LC.BOB_IP, LC.LINKS, LC.NOW
OPT_MSS_WS0 = LC.OPT_MSS_WS0  # <mss 1450,wscale 0>, as the connect scripts receive it
EXTRA = (SocketId.Udp((BOB, 5000)), SocketId.Passive((BOB, 80)))
server = LC.remote  # server k: (ip in octet order, port)


def lport(k: int) -> int:
    """The ephemeral port of row k."""
    return 49152 + k


def client(nrows: int, extra_flows=EXTRA, first: int = 0, **fields):
    """(flows, rows, con_map): row k connects from Bob's lport(first + k) to server(first + k); its Active flow follows
    `extra_flows` in the socket table."""
    ks = range(first, first + nrows)
    entries = list(extra_flows) + [SocketId.Active((BOB, lport(k)), (ipv4_str(server(k)[0]), server(k)[1])) for k in ks]
    flows = flow_array(entries)
    base = len(extra_flows)
    rows = TC.connector_table(nrows, flow_id=np.arange(base, base + nrows), local_ip=BOB_IP,
                              local_port=np.array([lport(k) for k in ks]),
                              remote_ip=np.array([server(k)[0] for k in ks], np.uint32),
                              remote_port=np.array([server(k)[1] for k in ks]), **fields)
    return flows, rows, TC.conn_of_flow(len(flows), rows)


def seg(k: int, flags: int, seq: int = 0, ack: int = 0, win: int = 65535, options: bytes = b"", payload: bytes = b"",
        **kw) -> bytes:
    """One frame from server k to the socket that connects to it."""
    s = server(k)
    return F.tcp_frame(payload=payload, src=s[0], dst=BOB, options=options, sport=s[1], dport=lport(k),
                       tcp_kw=dict(seq=seq & R.M32, ack=ack & R.M32, flags=flags, window=win), **kw)


def oracle_rx(frames_list, flows) -> dict:
    return LC.oracle_rx(frames_list, flows)


def started(rows: np.ndarray, nonce: int = 0, counter: int = 0, isn=R.crc_isn, now: int = NOW - 10, which=None):
    """A model whose rows `which` (all by default) have been through connect_start."""
    m = R.ConnectModel(rows, nonce, counter, isn)
    which = range(len(rows)) if which is None else which
    m.start(list(which), now, LINKS, slot_stride=64, max_frames=1 << 20, out_bytes=1 << 40, max_ready=1 << 20)
    return m


OTHER = [F.udp_frame(b"u" * 12, src="10.9.9.9", dst=BOB, sport=999, dport=5000),
         F.tcp_frame(src="10.9.9.8", dst=BOB, sport=5, dport=80, tcp_kw=dict(flags=SYN, seq=1)),  # the Passive flow
         F.tcp_frame(src="10.9.9.7", dst=BOB, sport=5, dport=lport(3), tcp_kw=dict(flags=SYN, checksum=0x1234)),
         F.tcp_frame(src="10.9.9.6", dst=BOB, sport=6, dport=9999, tcp_kw=dict(flags=SYN, seq=1))]  # no socket


def mixed_batch(seed: int = 5):
    """About 300 frames over 150 rows in every state, other traffic interleaved. Rows 0..139 are started (CONNECTING);
    the host then marks a few ESTABLISHED, FAILED and CLOSED; rows 140..149 stay IDLE. Returns (flows, rows, con_map,
    nonce, counter, patch, frames): `patch` maps row -> state to write after connect_start."""
    rng = np.random.default_rng(seed)
    nrows = 150
    flows, rows, cmap = client(nrows, window_scale=np.arange(nrows) % 15, link=np.arange(nrows) % 2,
                               handshake_retries=1 + np.arange(nrows) % 4,
                               receive_window_size=np.where(np.arange(nrows) % 7 == 0, 1000, 0xFFFF),
                               ip_word=np.where(np.arange(nrows) % 2, 0x00FF0000, 0x10400007))
    nonce, counter = 0xC0FFEE11, 0xFFC0
    m = started(rows, nonce, counter, which=range(140))
    isn = [int(x) for x in m.rows["local_isn"]]
    patch = {k: TC.ESTAB for k in range(100, 106)}
    patch.update({k: TC.FAILED for k in range(106, 110)})
    patch.update({k: TC.CLOSED for k in range(110, 113)})
    opts = [b"", bytes([2, 4, 5, 0xB4]), bytes([3, 3, 13]), bytes([3, 3, 15]), bytes([2, 4, 1, 0, 2, 4, 2, 0]),
            bytes([1, 2, 4, 4, 0, 1, 3, 3, 9, 1]), OPT_MSS_WS0]
    scripts = []
    for k in range(100):
        o, a, s0 = opts[k % len(opts)], isn[k] + 1, int(rng.integers(0, 1 << 32))
        kind = k % 10
        if kind == 0:    # accepted
            scripts.append([seg(k, SYN | ACK, seq=s0, ack=a, options=o, win=1 + k * 600)])
        elif kind == 1:  # refused
            scripts.append([seg(k, RST | ACK, seq=s0, ack=a)])
        elif kind == 2:  # a RST whose ack does not match: only an EAGAIN
            scripts.append([seg(k, RST | ACK, seq=s0, ack=a + 1)])
        elif kind == 3:  # SYN+RST with the right ack: refused
            scripts.append([seg(k, SYN | RST | ACK, seq=s0, ack=a, options=o)])
        elif kind == 4:  # the ACK bit clear with a matching ack_num: EAGAIN
            scripts.append([seg(k, SYN, seq=s0, ack=a, options=o)])
        elif kind == 5:  # a SYN+ACK carrying payload: accepted, the payload dropped
            scripts.append([seg(k, SYN | ACK, seq=s0, ack=a, options=o, payload=b"early data")])
        elif kind == 6:  # a plain ACK (no SYN): EAGAIN; then the SYN+ACK
            scripts.append([seg(k, ACK, seq=s0, ack=a), seg(k, SYN | ACK, seq=s0, ack=a, options=o)])
        elif kind == 7:  # accepted, then data behind it in the same batch
            scripts.append([seg(k, SYN | ACK, seq=s0, ack=a, options=o), seg(k, ACK | PSH, seq=s0 + 1, ack=a, payload=b"x")])
        elif kind == 8:  # strays until the SYNs run out, and one more
            scripts.append([seg(k, ACK, seq=s0, ack=a + 7)] * (int(rows["handshake_retries"][k]) + 1))
        else:            # refused, then more
            scripts.append([seg(k, RST | ACK, seq=s0, ack=a), seg(k, SYN | ACK, seq=s0, ack=a)])
    for k in range(100, 113):  # ESTABLISHED, FAILED, CLOSED rows
        scripts.append([seg(k, ACK | PSH, seq=1, ack=isn[k] + 1, payload=b"abc")] * 2)
    for k in range(140, 144):  # IDLE rows
        scripts.append([seg(k, SYN | ACK, seq=1, ack=1)])
    order = [si for si, s in enumerate(scripts) for _ in s]
    rng.shuffle(order)
    pos = [0] * len(scripts)
    frames = []
    for si in order:
        frames.append(scripts[si][pos[si]])
        pos[si] += 1
    k = 0
    while len(frames) < 301:
        frames.insert(int(rng.integers(0, len(frames))), OTHER[k % len(OTHER)])
        k += 1
    return flows, rows, cmap, nonce, counter, patch, frames


def find_row_with_big_crc(rows: np.ndarray, nonce: int, lo: int = 0xFFFF0000) -> int:
    """Rewrites row 0's remote so that its CRC exceeds `lo` and crc + counter wraps 2^32 (CPU search: about one in
    65,536, as tcp_listen_cases.find_remote_with_big_crc searches); returns the CRC."""
    row = rows[0].copy()
    for k in range(1, 1 << 22):
        row["remote_ip"] = ipv4(f"10.{(k >> 16) & 0xFF}.{(k >> 8) & 0xFF}.{1 + k % 250}")
        row["remote_port"] = 1024 + k % 60000
        crc = R.crc32_cksum(R.isn_bytes(row, nonce))
        if crc > lo:
            rows[0] = row
            return crc
    raise AssertionError("no such remote")
