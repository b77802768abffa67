"""A plain-Python restatement of the close coroutine (include/dk_tcp.h, the dk_tcp_close_* section): ControlBlock::close,
local_close and remote_already_closed (tcp/established/ctrlblk.rs:1039-1119) with process_ack (:607-650) and
process_remote_close (:1003-1026), one segment at a time per connection, the way the coroutine pops its recv_queue.
Deliberately not the device's parallel form: no minimum, no index comparison; a connection simply lives through its
frames in order. What Sender::process_ack and congestion control do with an accepted ACK is the existing kernels' part
(the ack_action hand-off) and is not restated here. The ACKs' bytes come from tests/tcp_ackemit_reference.py;
test_tcp_close_model.py pins this file against the reference's close scripts.
"""
from __future__ import annotations

import errno

import numpy as np

import tcp_ackemit_reference as AE
from demikernel_amd import _native as N
from demikernel_amd import tcp_close as TCL

M32, M64 = 0xFFFFFFFF, 2 ** 64 - 1
FIN, SYN, RST, PSH, ACK = 0x01, 0x02, 0x04, 0x08, 0x10
A = N.A


def le(a: int, b: int) -> bool:
    """SeqNumber's <= (sequence_number.rs:88-90): the sign of the wrapping difference."""
    d = (a - b) & M32
    return d == 0 or d >= 1 << 31


class Unreachable(Exception):
    """The reference's unreachable!() in local_close."""


class Block:
    """The part of one ControlBlock the close coroutine touches."""

    def __init__(self, state: int, snd_nxt: int, rcv_nxt: int):
        self.state, self.snd_nxt, self.rcv_nxt = state, snd_nxt, rcv_nxt
        self.acks = []      # RCV.NXT of every send_ack(), in order
        self.eof = False
        self.ack_ok = None  # process_ack's last result

    def send_ack(self):
        self.acks.append(self.rcv_nxt)

    def process_ack(self, flags: int, ack: int) -> bool:
        if not flags & ACK:
            return False
        # congestion control's on_ack_received runs here (the existing dk_tcp_cc_ack)
        if le(ack, self.snd_nxt):
            return True  # Sender::process_ack (the existing dk_tcp_ack_process)
        self.send_ack()
        return False

    def process_remote_close(self, flags: int) -> bool:
        if flags & FIN:
            self.eof = True
            self.rcv_nxt = (self.rcv_nxt + 1) & M32
            self.send_ack()
            return True
        return False

    def local_close_step(self, flags: int, ack: int):
        """One pass of local_close's loop (:1060-1092)."""
        self.ack_ok = self.process_ack(flags, ack)
        if self.ack_ok:
            if self.state == TCL.FIN_WAIT_1:
                self.state = TCL.FIN_WAIT_2
            elif self.state == TCL.FIN_WAIT_2:
                pass
            elif self.state == TCL.CLOSING:
                self.state = TCL.TIME_WAIT
            else:
                raise Unreachable(self.state)
        if self.process_remote_close(flags):
            if self.state == TCL.FIN_WAIT_1:
                self.state = TCL.CLOSING
            elif self.state == TCL.FIN_WAIT_2:
                self.state = TCL.TIME_WAIT
            else:
                raise Unreachable(self.state)

    def remote_already_closed_step(self, flags: int, ack: int):
        """One pass of remote_already_closed's loop (:1108-1117)."""
        self.ack_ok = self.process_ack(flags, ack)
        if self.ack_ok:
            self.state = TCL.CLOSED


def pop(b: Block, flags: int, ack: int) -> dict:
    """The coroutine of `b` pops one segment. The stated deviation: where the reference would panic (CLOSING + FIN)
    nothing of the frame is applied and the block is FAULT. -> what the frame did."""
    before = (b.state, b.rcv_nxt, len(b.acks), b.eof)
    try:
        if b.state == TCL.LAST_ACK:
            b.remote_already_closed_step(flags, ack)
        else:
            b.local_close_step(flags, ack)
    except Unreachable:
        b.state, b.rcv_nxt, b.eof = TCL.FAULT, before[1], before[3]
        del b.acks[before[2]:]
        return {"fault": True, "acks": [], "fin": False, "ack_ok": False, "unsent": False}
    acks = b.acks[before[2]:]
    fin = b.rcv_nxt != before[1]
    return {"fault": False, "acks": acks, "fin": fin, "ack_ok": b.ack_ok, "unsent": len(acks) > (1 if fin else 0)}


LIVE = (TCL.FIN_WAIT_1, TCL.FIN_WAIT_2, TCL.CLOSING, TCL.LAST_ACK)
ENDED = (TCL.TIME_WAIT, TCL.CLOSED, TCL.FAULT)


def row_check(Rx, T, nlinks: int, slot_stride: int, frame_lead: int) -> int:
    if int(Rx["state"]) != N.DK_TCP_CLOSED:
        return TCL.E_RX_STATE
    if int(T["state"]) != N.DK_TCP_ESTABLISHED:
        return TCL.E_STATE
    if int(T["link"]) >= nlinks:
        return TCL.E_LINK
    ws = int(T["rcv_wscale"])
    if ws > 14:
        return TCL.E_WSCALE
    if int(Rx["buffer_size"]) >> ws > 0xFFFF:
        return TCL.E_WINDOW
    if frame_lead + 54 > slot_stride:
        return TCL.E_SLOT
    return TCL.OK


def done_record(row: int, state: int, err: int, frame: int, fin_frame: int, deadline: int) -> np.ndarray:
    y = np.zeros(1, TCL.DONE_DTYPE)[0]
    y["row"], y["state"], y["err"], y["frame"], y["fin_frame"], y["deadline_ns"] = row, state, err, frame, fin_frame, deadline
    return y


class CloseModel:
    """The closer rows and the receive, send and delayed-ACK tables of the same connections (all copied)."""

    def __init__(self, rows, rx_conns, tx_conns, dack=None):
        self.rows, self.rx, self.tx = rows.copy(), rx_conns.copy(), tx_conns.copy()
        self.dack = None if dack is None else dack.copy()
        self.nconns = len(rows)

    def start(self, close) -> dict:
        """dk_tcp_close_start: close() up to its first await, entry by entry."""
        k = len(close)
        status = np.zeros(k, np.uint32)
        conn = np.full(k, 0xFFFFFFFF, np.uint32)
        m, top = 0, -1
        for j, c in enumerate(int(x) for x in close):
            if c >= self.nconns:
                st = TCL.E_ROW
            elif c <= top:
                st = TCL.E_ORDER
            elif int(self.tx["state"][c]) != N.DK_TCP_ESTABLISHED:
                st = TCL.E_STATE
            elif int(self.rows["state"][c]) != TCL.IDLE or int(self.rx["state"][c]) == N.DK_TCP_NONE:
                st = TCL.E_BADF
            else:
                st = TCL.OK
                R = self.rows[c]
                if int(self.rx["state"][c]) == N.DK_TCP_ESTABLISHED:
                    R["state"] = TCL.FIN_WAIT_1
                    self.rx["state"][c] = N.DK_TCP_CLOSED
                else:
                    R["state"] = TCL.LAST_ACK
                R["err"], R["flags"], R["deadline_ns"] = 0, 0, 0
                conn[m] = c
                m += 1
            top = max(top, c)
            status[j] = st
        z = np.zeros(k, np.uint32)
        return {"status": status, "conn": conn, "off": z, "len": z.copy(), "n_markers": m}

    def process(self, rx: dict, now_ns: int, links, *, slot_stride: int, frame_lead: int = 0, flags: int = 0,
                max_frames: int, out_bytes: int, max_done: int, action_in=None) -> dict:
        """dk_tcp_close_process over host arrays (rx: meta, flow_id, tcp_ack)."""
        n, nc = len(rx["meta"]), self.nconns
        status = np.zeros(nc, np.uint32)
        blocks = {}
        for c in range(nc):
            if int(self.rows["state"][c]) in LIVE:
                status[c] = row_check(self.rx[c], self.tx[c], len(links), slot_stride, frame_lead)
                if status[c] == TCL.OK:
                    blocks[c] = Block(int(self.rows["state"][c]), int(self.tx["snd_nxt"][c]), int(self.rx["receive_next"][c]))
        action, state_after = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        ack_action = np.zeros(n, np.uint8) if action_in is None else np.array(action_in, np.uint8, copy=True)
        reply_frame = np.full(n, TCL.NONE, np.uint32)
        fin_frame = np.full(nc, TCL.NONE, np.uint32)
        frames, frame_seg, done, work, sent = [], [], [], set(), set()
        for i in range(n):
            c = int(rx["flow_id"][i])
            if int(rx["meta"][i]) & 0xFF != N.V["OK_TCP"] or c >= nc or c not in blocks:
                continue
            b = blocks[c]
            work.add(c)
            if b.state in ENDED:  # the loop has ended: never popped
                action[i], state_after[i], ack_action[i] = TCL.UNPROCESSED, b.state, A["UNPROCESSED"]
                continue
            what = pop(b, (int(rx["meta"][i]) >> 16) & 0xFF, int(rx["tcp_ack"][i]))
            state_after[i] = b.state
            if what["fault"]:
                action[i], ack_action[i] = TCL.FAULT_BIT, A["UNPROCESSED"]
            else:
                action[i] = (TCL.POPPED | (TCL.ACK_OK if what["ack_ok"] else 0) | (TCL.ACK_UNSENT if what["unsent"] else 0) |
                             (TCL.FIN if what["fin"] else 0))
                ack_action[i] = A["NO_DATA"] if what["ack_ok"] else A["ACK_UNSENT"] if what["unsent"] else A["NO_ACK"]
                if what["fin"]:
                    fin_frame[c] = i
                T, Rx = self.tx[c], self.rx[c]
                for rn in what["acks"]:
                    if reply_frame[i] == TCL.NONE:
                        reply_frame[i] = len(frames)
                    wnd = (int(Rx["buffer_size"]) - ((rn - int(Rx["reader_next"])) & M32)) & M32
                    win = (wnd >> int(T["rcv_wscale"])) & 0xFFFF
                    frames.append(AE.ack_frame_bytes(T, links[int(T["link"])], rn, win, flags))
                    frame_seg.append(i)
                    sent.add(c)
            if b.state in ENDED:
                done.append((c, i))
        fits = len(frames) <= max_frames and len(frames) * slot_stride <= out_bytes and len(done) <= max_done
        exp = {"n_frames": len(frames), "n_done": len(done), "fits": fits}
        if not fits:
            for c in work:
                status[c] = TCL.NO_ROOM
            exp.update(status=status, frames=[], frame_seg=[], done=[])
            return exp
        recs = []
        for c, b in blocks.items():
            R = self.rows[c]
            if b.state != int(R["state"]):
                R["state"] = b.state
                if b.state == TCL.FAULT:
                    R["err"] = errno.EPROTO
                if b.state == TCL.TIME_WAIT:
                    R["deadline_ns"] = (now_ns + int(R["linger_ns"])) & M64
            self.rx["receive_next"][c] = b.rcv_nxt
            if c in sent and self.dack is not None:
                self.dack["armed"][c] = 0
        for c, i in done:
            R = self.rows[c]
            recs.append(done_record(c, int(R["state"]), int(R["err"]), i, int(fin_frame[c]), int(R["deadline_ns"])))
        exp.update(status=status, action=action, state_after=state_after, ack_action=ack_action, reply_frame=reply_frame,
                   fin_frame=fin_frame, frames=frames, frame_seg=frame_seg, done=recs)
        return exp

    def timers(self, now_ns: int, *, max_done: int, with_tx: bool = True) -> dict:
        """dk_tcp_close_timers: TIME-WAIT's end, and the retiring of closed rows."""
        due = [c for c in range(self.nconns)
               if int(self.rows["state"][c]) == TCL.TIME_WAIT and int(self.rows["deadline_ns"][c]) <= now_ns]
        rec = [c for c in range(self.nconns) if (c in due or int(self.rows["state"][c]) == TCL.CLOSED) and
               not int(self.rows["flags"][c]) & TCL.RETIRED]
        status = np.zeros(self.nconns, np.uint32)
        if len(rec) > max_done:
            status[sorted(set(due) | set(rec))] = TCL.NO_ROOM
            return {"n_done": len(rec), "status": status, "done": [], "fits": False}
        for c in due:
            self.rows["state"][c] = TCL.CLOSED
        recs = []
        for c in rec:
            R = self.rows[c]
            R["flags"] |= TCL.RETIRED
            if with_tx:
                self.tx["state"][c] = N.DK_TCP_CLOSED
            recs.append(done_record(c, TCL.CLOSED, int(R["err"]), TCL.NONE, TCL.NONE, int(R["deadline_ns"])))
        return {"n_done": len(rec), "status": status, "done": recs, "fits": True}


def blob_of(frames, slot_stride: int, frame_lead: int, size: int, fill: int) -> np.ndarray:
    """The output blob the device must leave: `fill` everywhere but the frames."""
    b = np.full(size, fill, np.uint8)
    for f, fr in enumerate(frames):
        o = f * slot_stride + frame_lead
        b[o:o + len(fr)] = np.frombuffer(fr, np.uint8)
    return b
