"""Case builder for the passive-open tests: a server (Bob) with listening sockets, remotes that send it frames, and the
batches the tests need. Frames are real Ethernet / IPv4 / TCP bytes (tests/frames.py); the receive results the model and
the device consume come from the receive oracle (CPU tests) or the receive engine (GPU tests) over the same bytes."""
from __future__ import annotations

import numpy as np

import frames as F
import tcp_listen_reference as R
import tx_segment_reference as M
from demikernel_amd import SocketId, flow_array, ipv4, synth
from demikernel_amd import tcp_listen as TL

FIN, SYN, RST, PSH, ACK = R.FIN, R.SYN, R.RST, R.PSH, R.ACK
BOB = synth.BOB_IPV4
BOB_IP = ipv4(BOB)
LINKS = M.links_table()
NOW = 5_000_000_000
OPT_MSS_WS0 = bytes([2, 4, 0x05, 0xAA, 3, 3, 0])  # <mss 1450,wscale 0>, as the accept scripts send it
OPT_NOP = bytes([1])


def remote(k: int) -> tuple:
    """Remote k: (ip in octet order, port)."""
    return ipv4(f"10.{1 + (k >> 8) % 200}.{k & 0xFF}.{1 + k % 250}"), 20000 + (k * 7) % 30000


def seg(rem: tuple, lport: int, flags: int, seq: int = 0, ack: int = 0, win: int = 65535, options: bytes = b"",
        payload: bytes = b"", **kw) -> bytes:
    """One frame from remote `rem` to Bob's port `lport`."""
    return F.tcp_frame(payload=payload, src=rem[0], dst=BOB, options=options, sport=rem[1], dport=lport,
                       tcp_kw=dict(seq=seq & R.M32, ack=ack & R.M32, flags=flags, window=win), **kw)


def server(ports, extra_flows=(), **fields):
    """(flows, listeners, lsn_map): one Passive flow and one listener row per port, after `extra_flows`."""
    entries = list(extra_flows) + [SocketId.Passive((BOB, p)) for p in ports]
    flows = flow_array(entries)
    first = len(extra_flows)
    fields.setdefault("max_backlog", 8)
    L = TL.listener_table(len(ports), flow_id=np.arange(first, first + len(ports)), local_ip=BOB_IP,
                          local_port=np.array(ports), **fields)
    return flows, L, TL.lsn_of_flow(len(flows), L)


def oracle_rx(frames_list, flows) -> dict:
    """The receive oracle's results for the frames (what dk_rx_process gives on the device)."""
    from oracle.oracle import OraclePeer

    blob, off, lens = F.pack(frames_list)
    peer = OraclePeer(BOB_IP)
    peer.set_flows(flows)
    return peer.process(blob, off, lens)


EXTRA = (SocketId.Udp((BOB, 5000)), SocketId.Active((BOB, 7000), ("10.250.0.9", 41000)))
ACTIVE_REMOTE = (ipv4("10.250.0.9"), 41000)


def isn_of(L_row, rem, counter: int) -> int:
    return (R.crc32_cksum(R.isn_bytes(L_row, rem[0], rem[1])) + (counter & 0xFFFF)) & R.M32


def mixed_batch(seed: int = 3):
    """293 frames (four whole waves and a part of one) for three listeners from about 40 remotes, other traffic
    interleaved, on top of a table that already holds SYN_RCVD, ESTABLISHED and FAILED entries (made by `warm`).
    Returns (flows, listeners, lsn_map, warm_frames, frames)."""
    rng = np.random.default_rng(seed)
    ports = [80, 443, 8080]
    flows, L, lsn = server(ports, EXTRA, max_backlog=[64, 64, 6], nonce=[0x1234, 0xCAFEF00D, 7],
                           window_scale=[0, 7, 14], isn_counter=[0, 0xFFF0, 5], link=[0, 1, 0])
    # warm: remotes 100.. get entries: 100-103 stay SYN_RCVD, 104-106 become ESTABLISHED, 107-108 FAILED
    warm = []
    counters = [int(c) for c in L["isn_counter"]]
    isn = {}
    for k in range(100, 109):
        li = k % 3
        rem = remote(k)
        warm.append(seg(rem, ports[li], SYN, seq=1000 * k, options=bytes([2, 4, 2, 0, 3, 3, k % 16, 0])))
        isn[k] = isn_of(L[li], rem, counters[li])
        counters[li] += 1
    for k in range(104, 107):
        warm.append(seg(remote(k), ports[k % 3], ACK, seq=1000 * k + 1, ack=isn[k] + 1))
    for k in range(107, 109):
        warm.append(seg(remote(k), ports[k % 3], ACK, seq=1000 * k + 1, ack=isn[k] + 7))
    # the batch: per-remote scripts, then shuffled together keeping each remote's own order
    scripts = []
    opts = [b"", bytes([2, 4, 5, 0xB4]), bytes([3, 3, 13]), bytes([3, 3, 14]), bytes([3, 3, 15]),
            bytes([2, 4, 1, 0, 2, 4, 2, 0]), bytes([1, 2, 4, 4, 0, 1, 3, 3, 9, 1]), OPT_MSS_WS0]
    for k in range(40):
        li, rem = k % 3, remote(k)
        p = ports[li]
        o = opts[k % len(opts)]
        kind = k % 10
        s0 = int(rng.integers(0, 1 << 32))
        if kind == 0:    # a SYN alone
            scripts.append([seg(rem, p, SYN, seq=s0, options=o)])
        elif kind == 1:  # a SYN and something behind it in the same batch: its ACK number is wrong unless by luck
            scripts.append([seg(rem, p, SYN, seq=s0, options=o), seg(rem, p, ACK, seq=s0 + 1, ack=12345)])
        elif kind == 2:  # two SYNs: the second is the handshake segment and fails it
            scripts.append([seg(rem, p, SYN, seq=s0, options=o), seg(rem, p, SYN, seq=s0, options=o),
                            seg(rem, p, ACK, seq=s0 + 1, ack=1)])
        elif kind == 3:  # non-SYN frames with and without ACK, then a RST
            scripts.append([seg(rem, p, PSH, seq=s0, options=o), seg(rem, p, ACK | PSH, seq=s0, ack=s0 ^ 0x5555,
                                                                      payload=b"x" * 9), seg(rem, p, RST, seq=s0)])
        elif kind == 4:  # a SYN with payload
            scripts.append([seg(rem, p, SYN, seq=s0, options=o, payload=b"hello")])
        elif kind == 5:  # SYN+ACK and RST+ACK to a listener; then a real SYN
            scripts.append([seg(rem, p, SYN | ACK, seq=s0, ack=77), seg(rem, p, RST | ACK, seq=s0, ack=0xFFFFFFFF),
                            seg(rem, p, SYN, seq=s0, options=o)])
        else:            # a SYN, other SYNs from the same remote later
            scripts.append([seg(rem, p, SYN, seq=s0, options=o)] + [seg(rem, p, FIN | ACK, seq=s0 + 1, ack=3)] * (kind - 5))
    # the right handshake ACKs for same-batch SYNs need the ISN: remotes 200.. on listener 0 get counters in order
    same = []
    for j, k in enumerate(range(200, 206)):
        same.append((k, seg(remote(k), ports[0], SYN, seq=77 * k, options=opts[j % len(opts)])))
    # frames for the warm entries
    for k in range(100, 102):
        scripts.append([seg(remote(k), ports[k % 3], ACK, seq=1000 * k + 1, ack=isn[k] + 1,
                            payload=b"data" if k & 1 else b""), seg(remote(k), ports[k % 3], ACK | PSH, seq=1000 * k + 1,
                                                                    ack=isn[k] + 1, payload=b"more")])
    scripts.append([seg(remote(102), ports[102 % 3], ACK, seq=5, ack=isn[102])])  # BAD_ACK, then ORPHANED
    scripts[-1].append(seg(remote(102), ports[102 % 3], ACK, seq=5, ack=isn[102] + 1))
    for k in range(104, 109):
        scripts.append([seg(remote(k), ports[k % 3], ACK | PSH, seq=1, ack=2, payload=b"abc")] * 2)
    other = [F.udp_frame(b"u" * 12, src="10.9.9.9", dst=BOB, sport=999, dport=5000),
             seg(ACTIVE_REMOTE, 7000, ACK | PSH, seq=1, ack=1, payload=b"active"),
             F.tcp_frame(src=remote(2)[0], dst=BOB, sport=5, dport=80, tcp_kw=dict(flags=SYN, checksum=0x1234)),
             seg(remote(3), 9999, SYN, seq=1)]
    order = [si for si, s in enumerate(scripts) for _ in s]
    rng.shuffle(order)
    pos = [0] * len(scripts)
    frames = []
    for si in order:
        frames.append(scripts[si][pos[si]])
        pos[si] += 1
    # the same-batch handshakes go in at fixed places so their counters are known: before every other SYN of listener 0
    head = [f for _, f in same]
    frames = head + frames
    c0 = counters[0]
    for j, (k, _) in enumerate(same):
        lisn = isn_of(L[0], remote(k), c0 + j)
        ackno = lisn + 1 if j != 3 else lisn + 2  # one of them is wrong
        frames.insert(len(head) + 10 * j + 5, seg(remote(k), ports[0], ACK, seq=77 * k + 1, ack=ackno,
                                                  payload=b"pay" if j == 1 else b""))
    k = 0
    while len(frames) < 293:  # other traffic, spread
        frames.insert(int(rng.integers(len(head), len(frames))), other[k % len(other)])
        k += 1
    assert len(frames) == 293, len(frames)
    return flows, L, lsn, warm, frames


def find_remote_with_big_crc(L_row, lo: int = 0xFFFF0000):
    """A remote whose CRC exceeds `lo`, so crc + counter wraps 2^32 (CPU search: about one in 65,536)."""
    for k in range(1, 1 << 22):
        rem = (ipv4(f"10.{(k >> 16) & 0xFF}.{(k >> 8) & 0xFF}.{1 + k % 250}"), 1024 + k % 60000)
        if R.crc32_cksum(R.isn_bytes(L_row, rem[0], rem[1])) > lo:
            return rem
    raise AssertionError("no such remote")


def colliding_remotes(cap: int, listener: int, homes, per_home: int):
    """Remotes whose keys' home slots are `homes` (per_home each), found by search with TL.home."""
    want = {h: [] for h in homes}
    k = 0
    while any(len(v) < per_home for v in want.values()):
        rem = remote(1000 + k)
        h = TL.home(cap, TL.key(listener, rem[0], rem[1]))
        if h in want and len(want[h]) < per_home and all(rem != r for v in want.values() for r in v):
            want[h].append(rem)
        k += 1
        assert k < 1 << 20
    return want
