"""A plain-Python restatement of the active open (include/dk_tcp.h, the dk_tcp_connect_* section): one frame at a
time against its row, the way SharedActiveOpenSocket::connect (tcp/active_open.rs) pops its recv_queue. Deliberately
not the device's parallel form: no counts, no ranks, no minimum; a row simply lives through its frames in order.

connect() is a loop of at most handshake_retries passes: send a SYN, wait for a segment or the timeout, run process_ack
on the segment. EAGAIN and the timeout both `continue`; when the passes run out the call fails with ECONNREFUSED. Here
syns_left counts the passes that remain after the SYN that is out. The frames' bytes come from tests/tx_reference.py;
test_tcp_connect_model.py pins this file against the reference's connect scripts.
"""
from __future__ import annotations

import errno

import numpy as np

import tx_reference as TR
from demikernel_amd import _native as N
from demikernel_amd import tcp_connect as TC
from tcp_listen_reference import crc32_cksum

M32, M64 = 0xFFFFFFFF, 2 ** 64 - 1
FIN, SYN, RST, PSH, ACK = 0x01, 0x02, 0x04, 0x08, 0x10


def isn_bytes(row, nonce: int) -> bytes:
    """What IsnGenerator::generate(local, remote) feeds the CRC (isn_generator.rs:31-37)."""
    return (int(row["remote_ip"]).to_bytes(4, "little") + int(row["remote_port"]).to_bytes(2, "big") +
            int(row["local_ip"]).to_bytes(4, "little") + int(row["local_port"]).to_bytes(2, "big") +
            int(nonce).to_bytes(4, "big"))


def crc_isn(row, nonce: int, counter: int) -> int:
    """The non-test build's generator: crc + counter."""
    return (crc32_cksum(isn_bytes(row, nonce)) + (counter & 0xFFFF)) & M32


def zero_isn(row, nonce: int, counter: int) -> int:
    """The reference's test build (isn_generator.rs:22-25): what the .pkt scripts were recorded with."""
    return 0


def row_check(row, nlinks: int, slot_stride: int, frame_lead: int) -> int:
    if int(row["window_scale"]) > 14:
        return TC.E_WSCALE
    if int(row["link"]) >= nlinks:
        return TC.E_LINK
    if frame_lead + TC.SYN_BYTES > slot_stride:
        return TC.E_SLOT
    return TC.OK


def frame_bytes(row, link_row, seq, ack, b13, options: bytes, flags: int) -> bytes:
    return TR.headers(b"", 6, int(row["local_ip"]), int(row["remote_ip"]),
                      int(row["local_port"]) | int(row["remote_port"]) << 16, meta=b13 << 16, seq=seq & M32, ack=ack & M32,
                      winurg=int(row["receive_window_size"]), options=options, ipw=int(row["ip_word"]),
                      dst_mac=bytes(link_row["dst_mac"]), src_mac=bytes(link_row["src_mac"]), flags=flags)


def syn_bytes(row, link_row, flags: int) -> bytes:
    opts = bytes([2, 4]) + int(row["advertised_mss"]).to_bytes(2, "big") + bytes([3, 3, int(row["window_scale"]), 0])
    return frame_bytes(row, link_row, int(row["local_isn"]), 0, SYN, opts, flags)


def ack_bytes(row, link_row, remote_seq: int, flags: int) -> bytes:
    return frame_bytes(row, link_row, int(row["local_isn"]) + 1, remote_seq + 1, ACK, b"", flags)


def error_record(r: int, row, cause: int, frame: int) -> np.ndarray:
    y = np.zeros(1, TC.READY_DTYPE)[0]
    y["row"], y["err"], y["cause"], y["frame"] = r, errno.ECONNREFUSED, cause, frame
    y["snd_nxt"] = (int(row["local_isn"]) + 1) & M32
    return y


def ready_record(r: int, row, rx: dict, i: int) -> np.ndarray:
    """The arguments of EstablishedSocket::new (active_open.rs:150-222)."""
    mss, rws = TC.FALLBACK_MSS, None
    if int(rx["meta"][i]) >> 28 > 5:
        rec = rx["tcp_opts"][i]
        for k in range(min(int(rec["num"]), 5)):
            o = rec["opt"][k]
            if o["kind"] == N.DK_TCPOPT_MSS:
                mss = int(o["u16"])
            elif o["kind"] == N.DK_TCPOPT_WS:
                rws = int(o["u8"])
    lws, rws = (0, 0) if rws is None else (int(row["window_scale"]), min(rws, 14))
    y = np.zeros(1, TC.READY_DTYPE)[0]
    y["row"], y["frame"] = r, i
    y["rcv_nxt"], y["snd_nxt"] = (int(rx["tcp_seq"][i]) + 1) & M32, (int(row["local_isn"]) + 1) & M32
    y["local_window"] = int(row["receive_window_size"]) << lws
    y["remote_window"] = (int(rx["tcp_win"][i]) & 0xFFFF) << rws
    y["mss"], y["local_wscale"], y["remote_wscale"] = mss, lws, rws
    return y


class ConnectModel:
    """The connector rows (a CONNECTOR_DTYPE array, copied) and the peer's ISN generator."""

    def __init__(self, rows: np.ndarray, nonce: int = 0, counter: int = 0, isn=crc_isn):
        self.rows = rows.copy()
        self.nonce, self.counter, self.isn = nonce, counter & 0xFFFF, isn

    @staticmethod
    def _fits(nf, nr, max_frames, slot_stride, out_bytes, max_ready) -> bool:
        return nf <= max_frames and nf * slot_stride <= out_bytes and nr <= max_ready

    def _eagain(self, R, r: int, now_ns: int, link_row, flags: int, frame: int):
        """The loop's `continue`: (action, SYN bytes or None, error record or None)."""
        if int(R["syns_left"]) > 0:
            R["syns_left"] -= 1
            R["deadline_ns"] = (now_ns + int(R["handshake_timeout_ns"])) & M64
            return TC.RETRY_SYN, syn_bytes(R, link_row, flags), None
        R["state"], R["err"] = TC.FAILED, errno.ECONNREFUSED
        return TC.EXHAUSTED, None, error_record(r, R, TC.CAUSE_EXHAUSTED, frame)

    def start(self, start, now_ns: int, links, *, slot_stride: int, frame_lead: int = 0, flags: int = 0,
              max_frames: int, out_bytes: int, max_ready: int) -> dict:
        rows = self.rows.copy()
        status, frames, frame_seg, ready, seen = [], [], [], [], set()
        for k, r in enumerate(int(x) for x in start):
            isn = self.isn(rows[r], self.nonce, self.counter + k) if r < len(rows) else 0  # generated before any check
            if r >= len(rows):
                status.append(TC.E_ROW)
                continue
            R = rows[r]
            dup = r in seen
            seen.add(r)
            if dup or R["state"] != TC.IDLE:
                status.append(TC.E_STATE)
                continue
            st = row_check(R, len(links), slot_stride, frame_lead)
            status.append(st)
            if st != TC.OK:
                continue
            R["local_isn"] = isn
            if int(R["handshake_retries"]) == 0:  # the loop body never runs: connect()'s last line
                R["state"], R["err"], R["syns_left"] = TC.FAILED, errno.ECONNREFUSED, 0
                ready.append(error_record(r, R, TC.CAUSE_EXHAUSTED, k))
                continue
            R["state"], R["err"] = TC.CONNECTING, 0
            R["syns_left"] = int(R["handshake_retries"]) - 1
            R["deadline_ns"] = (now_ns + int(R["handshake_timeout_ns"])) & M64
            frames.append(syn_bytes(R, links[int(R["link"])], flags))
            frame_seg.append(k)
        fits = self._fits(len(frames), len(ready), max_frames, slot_stride, out_bytes, max_ready)
        if fits:
            self.rows, self.counter = rows, (self.counter + len(start)) & 0xFFFF
        else:
            status = [TC.NO_ROOM if s == TC.OK else s for s in status]
        return {"fits": fits, "status": np.array(status, np.uint32), "n_frames": len(frames), "n_ready": len(ready),
                "frames": frames if fits else [], "frame_seg": frame_seg if fits else [], "ready": ready if fits else []}

    def process(self, rx: dict, con_map, now_ns: int, links, *, slot_stride: int, frame_lead: int = 0, flags: int = 0,
                max_frames: int, out_bytes: int, max_ready: int, link=None) -> dict:
        rows = self.rows.copy()
        nrows, n = len(rows), len(rx["meta"])
        status = [row_check(R, len(links), slot_stride, frame_lead) if R["state"] == TC.CONNECTING else TC.OK for R in rows]
        action, row_of, reply_frame = [TC.SKIP] * n, [TC.NONE] * n, [TC.NONE] * n
        frames, frame_seg, ready, work = [], [], [], set()
        for i in range(n):
            meta, f = int(rx["meta"][i]), int(rx["flow_id"][i])
            if meta & 0xFF != N.V["OK_TCP"] or f >= len(con_map):
                continue
            r = int(con_map[f])
            if r >= nrows:
                continue
            R = rows[r]
            if R["state"] in (TC.IDLE, TC.CLOSED) or status[r] != TC.OK:
                continue
            work.add(r)
            row_of[i] = r
            if R["state"] != TC.CONNECTING:  # the queue is the established socket's; a failed socket's entry is gone
                action[i] = TC.FORWARD if R["state"] == TC.ESTAB else TC.ORPHANED
                continue
            lk = int(R["link"])
            if link is not None and int(link[i]) < len(links):
                lk = int(link[i])
            fl = (meta >> 16) & 0xFF
            expected = (int(R["local_isn"]) + 1) & M32
            out_frame = rec = None
            if not (fl & ACK and int(rx["tcp_ack"][i]) == expected):        # process_ack :105
                action[i], out_frame, rec = self._eagain(R, r, now_ns, links[lk], flags, i)
            elif fl & RST:                                                   # :115
                R["state"], R["err"] = TC.FAILED, errno.ECONNREFUSED
                action[i], rec = TC.REFUSED, error_record(r, R, TC.CAUSE_RST, i)
            elif not fl & SYN:                                               # :122
                action[i], out_frame, rec = self._eagain(R, r, now_ns, links[lk], flags, i)
            else:
                action[i] = TC.ESTABLISHED
                out_frame = ack_bytes(R, links[lk], int(rx["tcp_seq"][i]), flags)
                rec = ready_record(r, R, rx, i)
                R["state"] = TC.ESTAB
            if out_frame is not None:
                reply_frame[i] = len(frames)
                frames.append(out_frame)
                frame_seg.append(i)
            if rec is not None:
                ready.append(rec)
        fits = self._fits(len(frames), len(ready), max_frames, slot_stride, out_bytes, max_ready)
        if fits:
            self.rows = rows
        else:
            status = [TC.NO_ROOM if status[r] == TC.OK and r in work else status[r] for r in range(nrows)]
        return {"fits": fits, "status": np.array(status, np.uint32), "n_frames": len(frames), "n_ready": len(ready),
                "frames": frames if fits else [], "frame_seg": frame_seg if fits else [], "ready": ready if fits else [],
                "action": np.array(action, np.uint8), "row": np.array(row_of, np.uint32),
                "reply_frame": np.array(reply_frame, np.uint32)}

    def timers(self, now_ns: int, links, *, slot_stride: int, frame_lead: int = 0, flags: int = 0, max_frames: int,
               out_bytes: int, max_ready: int) -> dict:
        """The pop's timeout (active_open.rs:275, :281), over the rows in ascending order."""
        rows = self.rows.copy()
        status, frames, frame_seg, ready, work = [], [], [], [], set()
        for r, R in enumerate(rows):
            st = row_check(R, len(links), slot_stride, frame_lead) if R["state"] == TC.CONNECTING else TC.OK
            status.append(st)
            if R["state"] != TC.CONNECTING or st != TC.OK or int(R["deadline_ns"]) > now_ns:
                continue
            work.add(r)
            _, fr, rec = self._eagain(R, r, now_ns, links[int(R["link"])], flags, TC.NONE)
            if fr is not None:
                frames.append(fr)
                frame_seg.append(r)
            else:
                ready.append(rec)
        fits = self._fits(len(frames), len(ready), max_frames, slot_stride, out_bytes, max_ready)
        if fits:
            self.rows = rows
        else:
            status = [TC.NO_ROOM if status[r] == TC.OK and r in work else status[r] for r in range(len(rows))]
        return {"fits": fits, "status": np.array(status, np.uint32), "n_frames": len(frames), "n_ready": len(ready),
                "frames": frames if fits else [], "frame_seg": frame_seg if fits else [], "ready": ready if fits else []}


def blob_of(frames, slot_stride: int, frame_lead: int, size: int, fill: int) -> np.ndarray:
    """The output blob the device must leave: `fill` everywhere but the frames."""
    b = np.full(size, fill, np.uint8)
    for f, fr in enumerate(frames):
        o = f * slot_stride + frame_lead
        b[o:o + len(fr)] = np.frombuffer(fr, np.uint8)
    return b
