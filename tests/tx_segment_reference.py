"""TEST INFRASTRUCTURE ONLY: a plain-Python restatement of the reference's send loop, for the dk_tcp_tx_segment tests to
compare against byte for byte.

    Sender::get_open_window_size_bytes / send_segment   layer4/tcp/established/sender.rs:124-208
    ControlBlock::tcp_header, hdr_window_size            layer4/tcp/established/ctrlblk.rs:699-709, :786-803

`segment` is literally that loop, one segment at a time per connection with no ACK arriving meanwhile (not the closed
form the kernels use), plus dk_tcp_tx_segment's batch contract (include/dk_tcp.h): the connection-level failures, the
statuses, the frame numbering and the all-or-nothing capacity rule. Header bytes come from tests/tx_reference.py.
tests/test_tcp_tx_segment_model.py pins this module against hand-written cases and the receive oracles.
"""
from __future__ import annotations

import numpy as np

import tx_reference as R

SENT, PARTIAL, UNSENT, CLOSED, E_CONN, NO_ROOM = range(6)
ESTABLISHED = 1
FIN, PSH, ACK = 0x01, 0x08, 0x10
M32 = 0xFFFFFFFF
MAX_MSS = 65481  # 54 + mss, the whole frame, must fit the 16-bit len_out (dk_rx_batch.len)


def open_window(snd_una: int, snd_nxt: int, snd_wnd: int, cwnd: int, mss: int) -> int:
    """get_open_window_size_bytes (sender.rs:124-147) with the effective cwnd given."""
    sent = (snd_nxt - snd_una) & M32
    if snd_wnd > 0 and snd_wnd >= sent and cwnd >= sent:
        return min(snd_wnd - sent, mss, cwnd - sent)
    return 0


def send_segment(remaining: int, marker: bool, c: dict):
    """send_segment (sender.rs:151-208) on a buffer with `remaining` bytes left (marker: the zero-length end-of-send
    buffer). c: snd_una, snd_nxt, snd_wnd, cwnd, mss; snd_nxt advances. Returns None when the window is closed, else
    (payload bytes, seq, tcp flags, sequence space consumed)."""
    size = open_window(c["snd_una"], c["snd_nxt"], c["snd_wnd"], c["cwnd"], c["mss"])
    if size == 0:
        return None
    if remaining > size:
        nbytes, flags = size, ACK  # PSH suppressed for partial buffers
    else:
        # a zero-length segment is the end-of-send marker: FIN; else the piece that ends the buffer carries PSH
        nbytes, flags = remaining, ACK | (FIN if remaining == 0 else PSH)
    seq = c["snd_nxt"]
    consumed = nbytes if nbytes else 1  # the FIN takes one sequence number
    c["snd_nxt"] = (seq + consumed) & M32
    return nbytes, seq, flags, consumed


def header_window(rx, wscale: int):
    """hdr_window_size (ctrlblk.rs:786-803) of a dk_tcp_conn record; None where its expect_ok! would panic."""
    unread = (int(rx["receive_next"]) - int(rx["reader_next"])) & M32
    w = ((int(rx["buffer_size"]) - unread) & M32) >> wscale if wscale <= 31 else 0
    return w if w <= 0xFFFF else None


def segment(src: np.ndarray, conn, off, lens, tx_conns: np.ndarray, links: np.ndarray, out: np.ndarray, *,
            slot_stride: int, frame_lead: int, max_frames: int, rx_conns=None, flags: int = 0, src_bytes=None,
            out_bytes=None) -> dict:
    """dk_tcp_tx_segment over host arrays. Returns the new `out` and `tx_conns` (copies) and every result array
    (per-frame arrays hold the frames written: none when the call ran out of room)."""
    out = np.array(out, np.uint8, copy=True)
    tx = np.array(tx_conns, copy=True)
    sb = src.size if src_bytes is None else src_bytes
    ob = out.size if out_bytes is None else out_bytes
    nb, nc = len(conn), len(tx)
    conn, off, lens = (np.asarray(a, np.uint32) for a in (conn, off, lens))
    assert np.all(np.diff(conn.astype(np.int64)) >= 0), "conn must be non-decreasing"
    sent, first, count, status = (np.zeros(nb, np.uint32) for _ in range(4))
    frames = []  # (buffer, source offset, bytes, seq, tcp flags, ack, window, connection)
    commits = []  # (connection, snd_nxt, fin_sent)
    i = 0
    while i < nb:
        c = int(conn[i])
        e = i
        while e < nb and conn[e] == c:
            e += 1
        bufs = range(i, e)
        i = e
        for b in bufs:
            first[b] = len(frames)
        T = tx[c] if c < nc else None
        ack = win = 0
        ok = T is not None and int(T["state"]) == ESTABLISHED
        if ok:
            ack, win = int(T["rcv_nxt"]), int(T["rcv_wnd_hdr"])
            if rx_conns is not None:
                ack, win = int(rx_conns[c]["receive_next"]), header_window(rx_conns[c], int(T["rcv_wscale"]))
            ok = (win is not None and int(T["link"]) < len(links) and int(T["mss"]) <= MAX_MSS and
                  frame_lead + 54 + int(T["mss"]) <= slot_stride and
                  all(int(off[b]) + int(lens[b]) <= sb for b in bufs))
        if not ok:
            status[list(bufs)] = E_CONN
            continue
        cb = {k: int(T[k]) for k in ("snd_una", "snd_nxt", "snd_wnd", "cwnd", "mss")}
        fin_sent, marker_seen = bool(T["fin_sent"]), False
        for b in bufs:
            first[b] = len(frames)
            if fin_sent or marker_seen:
                status[b] = CLOSED
                continue
            total, marker = int(lens[b]), int(lens[b]) == 0
            marker_seen = marker
            remaining, done = total, False
            while not done:
                r = send_segment(remaining, marker, cb)
                if r is None:
                    break  # the connection stops: nothing moves SND.UNA inside the call
                nbytes, seq, fl, consumed = r
                frames.append((b, int(off[b]) + total - remaining, nbytes, seq, fl, ack, win, c))
                remaining -= nbytes
                sent[b] += consumed
                count[b] += 1
                done = bool(fl & (PSH | FIN))
            fin_sent = done and marker
            status[b] = SENT if done else PARTIAL if sent[b] else UNSENT
        commits.append((c, cb["snd_nxt"], fin_sent))
    need = len(frames)
    res = {"n_frames": need, "first_frame": first, "frame_count": count}
    if need > max_frames or need * slot_stride > ob:
        status[count > 0] = NO_ROOM
        sent[:] = 0
        frames = []
    else:
        for c, nxt, fin in commits:
            tx["snd_nxt"][c] = nxt
            if fin:
                tx["fin_sent"][c] = 1
    n = len(frames)
    off_out, len_out, frame_buf = np.zeros(n, np.uint32), np.zeros(n, np.uint16), np.zeros(n, np.uint32)
    for f, (b, so, nbytes, seq, fl, ack, win, c) in enumerate(frames):
        T = tx[c]
        payload = src[so:so + nbytes].tobytes()
        link = links[int(T["link"])]
        h = R.headers(payload, 6, int(T["local_ip"]), int(T["remote_ip"]), int(T["ports"]),
                      meta=6 << 8 | fl << 16 | 5 << 28, seq=seq, ack=ack, winurg=win, ipw=int(T["ip_word"]),
                      dst_mac=bytes(link["dst_mac"]), src_mac=bytes(link["src_mac"]), flags=flags)
        a = f * slot_stride + frame_lead
        out[a:a + 54 + nbytes] = np.frombuffer(h + payload, np.uint8)
        off_out[f], len_out[f], frame_buf[f] = a, 54 + nbytes, b
    res.update(out=out, tx_conns=tx, off_out=off_out, len_out=len_out, frame_buf=frame_buf, sent=sent, status=status)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# Builders shared by the CPU and GPU tests.
# ---------------------------------------------------------------------------------------------------------------------
def links_table():
    from demikernel_amd import synth, tx_links

    return tx_links([(synth.BOB_MAC, synth.ALICE_MAC), (bytes([2, 0, 0, 0xAA, 0xBB, 0xCC]), bytes([0xFE, 1, 2, 3, 4, 5]))])


def conns_toward(flows, seed: int = 5, **kw) -> np.ndarray:
    """Send sides (TX_CONN_DTYPE) of the remote ends of a receiving peer's Active flows (FLOW_DTYPE): connection c sends
    to flow c of that peer. Random SND.NXT / RCV.NXT / header window / identification unless given in kw
    (tx_conn_table's arguments)."""
    from demikernel_amd.tcp_tx import tx_conn_table

    rng = np.random.default_rng(seed)
    n = len(flows)
    u32 = lambda: rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    args = dict(snd_nxt=u32(), rcv_nxt=u32(), rcv_wnd_hdr=rng.integers(0, 65536, n).astype(np.uint16),
                snd_wnd=1 << 30, mss=1460, local_ip=flows["remote_ip"], remote_ip=flows["local_ip"],
                ports=flows["remote_port"].astype(np.uint32) | flows["local_port"].astype(np.uint32) << 16,
                ip_word=(rng.integers(0, 65536, n) | rng.integers(1, 256, n) << 16 | rng.integers(0, 256, n) << 24),
                link=rng.integers(0, 2, n))
    args.update(kw)
    return tx_conn_table(n, **args)


def pack_push(conn, lens, residues=None, seed: int = 9):
    """A source blob of random bytes and the push arrays for buffers of `lens` bytes on connections `conn`
    (non-decreasing). residues: each buffer's source offset mod 16 (default: packed back to back)."""
    rng = np.random.default_rng(seed)
    off, pos = [], 0
    for i, l in enumerate(lens):
        if residues is not None:
            pos += (int(residues[i]) - pos) % 16
        off.append(pos)
        pos += int(l)
    src = rng.integers(0, 256, max(pos, 1) + 3, dtype=np.uint8)
    return src, np.asarray(conn, np.uint32), np.asarray(off, np.uint32), np.asarray(lens, np.uint32)
