"""TEST INFRASTRUCTURE ONLY: a plain-Python restatement of dk_tcp_ack_emit and dk_tcp_ack_timer (include/dk_tcp.h) for
the tests to compare against byte for byte.

    ControlBlock::process_packet and what it calls    layer4/tcp/established/ctrlblk.rs:403-695, :836-1024
    ControlBlock::send_ack, tcp_header, emit          ctrlblk.rs:699-776
    hdr_window_size                                   ctrlblk.rs:786-803
    the delayed-ACK expiry                            layer4/tcp/established/background/acknowledger.rs

`ack_emit` is the literal loop: one segment at a time, in arrival order, through a process_packet that keeps RCV.NXT,
the out-of-order store and the delayed-ACK deadline itself and sends each ACK where the reference sends it, with the
RCV.NXT and window of that moment. It does not use the engine's actions or its order by connection; its own actions,
views and final table are pinned against the receive oracle by tests/test_tcp_ackemit_model.py. On top sits the batch
contract of dk_tcp.h: the connection-level failures, the frame numbering and the all-or-nothing capacity rule. Header
bytes come from tests/tx_reference.py with the descriptor tests/tx_segment_reference.py uses.
"""
from __future__ import annotations

import numpy as np

import tx_reference as R
import tx_segment_reference as M

M32 = 0xFFFFFFFF
OK, E_STATE, E_SND_NXT, E_LINK, E_WSCALE, E_WINDOW, E_SLOT, NO_ROOM, NOT_FIRED, IDLE = range(10)
NO_FRAME = 0xFFFFFFFF
NONE, ESTABLISHED, CLOSED = 0, 1, 2
(SKIP, DELIVERED, STORED, STORE_DUP, NO_DATA, FIN_, DUPLICATE, OUT_OF_WINDOW, RST_, SYN_, NO_ACK, ACK_UNSENT,
 UNPROCESSED) = range(13)
F_FIN, F_SYN, F_RST, F_ACK = 0x01, 0x02, 0x04, 0x10
OOO_MAX = 16
V_OK_TCP = 0
DACK_DTYPE = np.dtype([("armed", "<u4"), ("reserved", "<u4"), ("delay_ns", "<u8"), ("deadline_ns", "<u8"),
                       ("reserved1", "<u8")])
VIEW_DTYPE = np.dtype([("ref", "<u4"), ("off", "<u4"), ("len", "<u4")])


def lt(a: int, b: int) -> bool:
    """SeqNumber's `<` (sequence_number.rs:76-101): the sign of the wrapping difference."""
    return ((a - b) & M32) >= 0x80000000


def le(a: int, b: int) -> bool:
    return a == b or lt(a, b)


class Conn:
    """The receive half of one ControlBlock plus its delayed-ACK deadline."""

    def __init__(self, row, armed: bool):
        self.state, self.rn, self.reader = int(row["state"]), int(row["receive_next"]), int(row["reader_next"])
        self.bufsz, self.snd = int(row["buffer_size"]), int(row["send_next"])
        self.fin_pending, self.fin_seq = int(row["fin_pending"]), int(row["fin_seq"])
        k = min(int(row["ooo_count"]), OOO_MAX)
        self.ooo = [(int(row["ooo_start"][j]), [int(row["ooo"][j][f]) for f in ("ref", "off", "len")]) for j in range(k)]
        self.armed, self.touched, self.armed_once = armed, False, False
        self.acks = []  # (triggering frame, RCV.NXT, window before the scale shift) per ACK sent

    def window(self) -> int:
        return (self.bufsz - ((self.rn - self.reader) & M32)) & M32

    def write(self, row) -> None:
        row["state"], row["receive_next"] = self.state, self.rn
        row["fin_pending"], row["fin_seq"], row["ooo_count"] = self.fin_pending, self.fin_seq, len(self.ooo)
        for j in range(OOO_MAX):
            st, v = self.ooo[j] if j < len(self.ooo) else (0, [0, 0, 0])
            row["ooo_start"][j] = st
            row["ooo"][j] = tuple(v)

    # ---- the delayed-ACK deadline ----
    def send_ack(self, i: int) -> None:
        """send_ack -> emit: the frame, then the deadline is cleared (ctrlblk.rs:761)."""
        self.acks.append((i, self.rn, self.window()))
        self.armed, self.touched = False, True

    def arm(self) -> None:
        self.armed, self.touched, self.armed_once = True, True, True

    # ---- the out-of-order store (ctrlblk.rs:836-941) ----
    def store(self, start: int, end: int, view: list) -> int:
        again = True
        while again:
            again = False
            at = len(self.ooo)
            for k, (ss, sv) in enumerate(self.ooo):
                se = (ss + sv[2] - 1) & M32
                if lt(start, ss):
                    if lt(end, ss):
                        at = k
                        break
                    if lt(se, end):  # the new segment covers the stored one: drop that and look again
                        again, at = True, k
                        break
                    excess = ((end - ss) & M32) + 1  # overlaps its front: cut, and inserted at the back (the quirk)
                    end = (end - excess) & M32
                    view[2] -= excess
                    break
                if le(end, se):
                    return STORE_DUP
                if lt(se, start):
                    continue
                dup = (se - start) & M32  # overlaps its end: one byte short (the quirk, ctrlblk.rs:916)
                start = (start + dup) & M32
                view[1] += dup
                view[2] -= dup
            if again:
                del self.ooo[at]
        if at < OOO_MAX:
            self.ooo.insert(at, (start, view))
            del self.ooo[OOO_MAX:]
        return STORED

    def receive_data(self, view: list) -> bool:
        """receive_data (ctrlblk.rs:951-1001): True if a stored FIN is now in order."""
        nxt = (self.rn + view[2]) & M32
        self.rn = nxt
        while self.ooo and self.ooo[0][0] == nxt:
            _, v = self.ooo.pop(0)
            nxt = (nxt + v[2]) & M32
            self.rn = nxt
        return bool(self.fin_pending) and self.fin_seq == nxt

    # ---- process_packet (ctrlblk.rs:403-440) ----
    def process(self, i: int, seq: int, ack: int, flags: int, pay_off: int, pay_len: int):
        """-> (action, view). Sends the segment's ACK, if any, through send_ack at the point the reference does."""
        syn, fin, rst, has_ack = bool(flags & F_SYN), bool(flags & F_FIN), bool(flags & F_RST), bool(flags & F_ACK)
        view = [i, pay_off, pay_len]
        start, seg_len = seq, pay_len + syn + fin
        end = (start + seg_len - 1) & M32 if seg_len else start
        after = (self.rn + self.window()) & M32
        if start != self.rn:
            if lt(start, self.rn):
                if lt(end, self.rn):  # entirely old (ctrlblk.rs:495-504)
                    if not rst:
                        self.send_ack(i)
                    return DUPLICATE, [i, pay_off, pay_len]
                dup = (self.rn - start) & M32
                start, seg_len = (start + dup) & M32, seg_len - dup
                if syn:
                    syn, dup = False, dup - 1
                view[1] += dup
                view[2] -= dup
            elif not lt(start, after):  # beyond the window (ctrlblk.rs:525-535)
                if not rst:
                    self.send_ack(i)
                return OUT_OF_WINDOW, [i, pay_off, pay_len]
        if seg_len > 0 and not lt(end, after):
            excess = ((end - after) & M32) + 1
            end, seg_len = (end - excess) & M32, seg_len - excess
            if fin:
                fin, excess = False, excess - 1
            view[2] -= excess
        out_view = list(view)
        if rst:
            self.state = CLOSED
            return RST_, out_view
        if syn:
            return SYN_, out_view
        if not has_ack:
            return NO_ACK, out_view
        if not le(ack, self.snd):  # acknowledges what was never sent (ctrlblk.rs:640-647)
            self.send_ack(i)
            return ACK_UNSENT, out_view
        action = NO_DATA
        if view[2] > 0 or fin:  # process_data (ctrlblk.rs:652-695)
            if start != self.rn:
                action = STORED
                if seg_len > 0:
                    if fin:
                        seg_len -= 1
                        self.fin_pending, self.fin_seq = 1, end
                        end = (end - 1) & M32
                        fin = False
                    if seg_len > 0:
                        action = self.store(start, end, view)
                    self.send_ack(i)  # ctrlblk.rs:680-682: the peer learns of the hole at once
            else:
                action = DELIVERED
                if self.receive_data(view):
                    fin = True
        if fin:  # process_remote_close (ctrlblk.rs:1003-1024): returns before the deadline is looked at
            self.rn = (self.rn + 1) & M32
            self.state = CLOSED
            self.send_ack(i)
            return FIN_, out_view
        if not self.armed:  # ctrlblk.rs:426-437
            self.arm()
        else:
            self.send_ack(i)
        return action, out_view


def check_conn(T, Rx, nlinks: int, slot_stride: int, frame_lead: int) -> int:
    """The connection-level checks in dk_tcp.h's order."""
    if int(T["state"]) != ESTABLISHED:
        return E_STATE
    if int(Rx["send_next"]) != int(T["snd_nxt"]):
        return E_SND_NXT
    if int(T["link"]) >= nlinks:
        return E_LINK
    ws = int(T["rcv_wscale"])
    if ws > 14:
        return E_WSCALE
    if int(Rx["buffer_size"]) >> ws > 0xFFFF:
        return E_WINDOW
    if frame_lead + 54 > slot_stride:
        return E_SLOT
    return OK


def ack_frame_bytes(T, link, ack: int, win: int, flags: int) -> bytes:
    return R.headers(b"", 6, int(T["local_ip"]), int(T["remote_ip"]), int(T["ports"]),
                     meta=6 << 8 | M.ACK << 16 | 5 << 28, seq=int(T["snd_nxt"]), ack=ack, winurg=win,
                     ipw=int(T["ip_word"]), dst_mac=bytes(link["dst_mac"]), src_mac=bytes(link["src_mac"]), flags=flags)


def _write_frames(out, desc, tx, links, flags, slot_stride, frame_lead):
    """desc: (item, connection, RCV.NXT, unscaled window) per frame -> off_out, len_out, frame_conn, frame_seg."""
    n = len(desc)
    off_out, len_out = np.zeros(n, np.uint32), np.zeros(n, np.uint16)
    frame_conn, frame_seg = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for f, (item, c, rn, wnd) in enumerate(desc):
        T = tx[c]
        win = (wnd >> int(T["rcv_wscale"])) & 0xFFFF
        a = f * slot_stride + frame_lead
        out[a:a + 54] = np.frombuffer(ack_frame_bytes(T, links[int(T["link"])], rn, win, flags), np.uint8)
        off_out[f], len_out[f], frame_conn[f], frame_seg[f] = a, 54, c, item
    return off_out, len_out, frame_conn, frame_seg


def ack_emit(rx: dict, rx_conns: np.ndarray, tx_conns: np.ndarray, dack: np.ndarray, links: np.ndarray, now_ns: int,
             out: np.ndarray, *, slot_stride: int, frame_lead: int = 0, max_frames: int, flags: int = 0,
             out_bytes=None) -> dict:
    """dk_tcp_rx_process followed by dk_tcp_ack_emit over host arrays. rx: the dk_rx results meta, flow_id, tcp_seq,
    tcp_ack, payload; rx_conns: the table before dk_tcp_rx_process. Returns copies of `out`, `dack` and the receive
    table after the call, the segments' actions and views, every result array (per-frame arrays hold the frames
    written: none when the call ran out of room) and `desc`, the planned frames as (batch frame, connection, RCV.NXT,
    window before the scale shift)."""
    out = np.array(out, np.uint8, copy=True)
    dk = np.array(dack, copy=True)
    table = np.array(rx_conns, copy=True)
    n, nc = len(rx["meta"]), len(table)
    ob = out.size if out_bytes is None else out_bytes
    conns = [Conn(table[c], bool(dk["armed"][c])) for c in range(nc)]
    action = np.zeros(n, np.uint8)
    view = np.zeros(n, VIEW_DTYPE)
    for i in range(n):
        meta, f, pay = int(rx["meta"][i]), int(rx["flow_id"][i]), int(rx["payload"][i])
        view[i] = (i, pay & 0xFFFF, pay >> 16)
        if (meta & 0xFF) != V_OK_TCP or f >= nc or conns[f].state == NONE:
            continue
        k = conns[f]
        if k.state != ESTABLISHED:  # queued behind the close: never processed (ctrlblk.rs:355-363)
            action[i] = UNPROCESSED
            continue
        act, v = k.process(i, int(rx["tcp_seq"][i]), int(rx["tcp_ack"][i]), (meta >> 16) & 0xFF, pay & 0xFFFF, pay >> 16)
        action[i], view[i] = act, tuple(v)
    for c in range(nc):
        conns[c].write(table[c])
    # the batch contract
    status = np.array([check_conn(tx_conns[c], rx_conns[c], len(links), slot_stride, frame_lead) for c in range(nc)],
                      np.uint32).reshape(nc)
    n_acks = np.zeros(nc, np.uint32)
    desc = []
    for c in range(nc):
        if status[c] == OK:
            n_acks[c] = len(conns[c].acks)
            desc += [(i, c, rn, wnd) for i, rn, wnd in conns[c].acks]
    desc.sort()  # by the batch frame that triggered it
    need = len(desc)
    fits = need <= max_frames and need * slot_stride <= ob
    ack_frame = np.full(n, NO_FRAME, np.uint32)
    if fits:
        for f, d in enumerate(desc):
            ack_frame[d[0]] = f
        for c in range(nc):
            k = conns[c]
            if status[c] != OK:
                continue
            if k.touched:
                dk["armed"][c] = int(k.armed)
            if k.armed_once:
                dk["deadline_ns"][c] = (now_ns + int(dk["delay_ns"][c])) & 0xFFFFFFFFFFFFFFFF
    else:
        status[(status == OK) & (n_acks > 0)] = NO_ROOM
    off_out, len_out, frame_conn, frame_seg = _write_frames(out, desc if fits else [], tx_conns, links, flags,
                                                            slot_stride, frame_lead)
    return dict(out=out, dack=dk, rx_conns=table, action=action, view=view, status=status, n_acks=n_acks,
                ack_frame=ack_frame, n_frames=need, off_out=off_out, len_out=len_out, frame_conn=frame_conn,
                frame_seg=frame_seg, desc=desc)


def ack_timer(fire, tx_conns: np.ndarray, rx_conns: np.ndarray, dack: np.ndarray, links: np.ndarray, out: np.ndarray, *,
              slot_stride: int, frame_lead: int = 0, max_frames: int, flags: int = 0, out_bytes=None) -> dict:
    """dk_tcp_ack_timer over host arrays: the acknowledger's expiry for the connections `fire` names."""
    out = np.array(out, np.uint8, copy=True)
    dk = np.array(dack, copy=True)
    fire = np.asarray(fire, np.uint8)
    nc = len(fire)
    ob = out.size if out_bytes is None else out_bytes
    status = np.full(nc, NOT_FIRED, np.uint32)
    desc = []
    for c in range(nc):
        if not fire[c]:
            continue
        status[c] = check_conn(tx_conns[c], rx_conns[c], len(links), slot_stride, frame_lead)
        if status[c] == OK and not int(dk["armed"][c]):
            status[c] = IDLE
        if status[c] == OK:
            k = Conn(rx_conns[c], True)
            desc.append((c, c, k.rn, k.window()))
    need = len(desc)
    fits = need <= max_frames and need * slot_stride <= ob
    ack_frame = np.full(nc, NO_FRAME, np.uint32)
    n_acks = np.zeros(nc, np.uint32)
    for f, d in enumerate(desc):
        n_acks[d[0]] = 1
        if fits:
            ack_frame[d[0]] = f
            dk["armed"][d[0]] = 0
        else:
            status[d[0]] = NO_ROOM
    off_out, len_out, frame_conn, _ = _write_frames(out, desc if fits else [], tx_conns, links, flags, slot_stride,
                                                    frame_lead)
    return dict(out=out, dack=dk, status=status, n_acks=n_acks, ack_frame=ack_frame, n_frames=need, off_out=off_out,
                len_out=len_out, frame_conn=frame_conn, desc=desc)
