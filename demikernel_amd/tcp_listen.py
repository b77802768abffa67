"""The passive open on the GPU (include/dk_tcp.h, the dk_tcp_listen_* section).

What SharedPassiveSocket does with the frames that reach a listening socket (tcp/passive_open.rs): the lookup in
`connections`, the SYN test, the backlog check and the ISN, the SYN+ACK with its options, the RST for everything else,
the handshake ACK and its timeout, for every listener-bound frame of one RxEngine.receive_batch call at once. The
connections of all listeners live in one device table (ListenTable) that the device inserts into; the listeners are
rows of LISTENER_DTYPE. A ready record carries what EstablishedSocket::new receives; conn_rows_from_ready turns one into
rows of the established-state tables.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native as N
from .rx import RxResults, _check, _ptr

LISTENER_DTYPE, SLOT_DTYPE, READY_DTYPE = N.LISTENER_DTYPE, N.LSN_SLOT_DTYPE, N.LSN_READY_DTYPE
ACTIONS, STATUSES, SLOT_STATES = N.TCP_LSN_ACTIONS, N.TCP_LSN_STATUSES, N.TCP_LSN_SLOT_STATES
(SKIP, SYN_ACCEPTED, ESTABLISHED, ESTABLISHED_DATA, BAD_ACK, FORWARD, ORPHANED, RST_FLAGS, RST_BACKLOG) = range(9)
OK, E_WSCALE, E_LINK, E_SLOT, E_TABLE, NO_ROOM = range(6)
FREE, SYN_RCVD, ESTAB, FAILED, TOMBSTONE = range(5)
NONE = N.DK_TCP_LSN_NONE
NO_WSCALE = N.DK_TCP_LSN_NO_WSCALE
FALLBACK_MSS = N.DK_TCP_LSN_FALLBACK_MSS
SYNACK_BYTES, RST_BYTES = N.DK_TCP_LSN_SYNACK_BYTES, N.DK_TCP_LSN_RST_BYTES
KEY_FREE, KEY_TOMBSTONE = N.DK_TCP_LSN_KEY_FREE, N.DK_TCP_LSN_KEY_TOMBSTONE


def listener_table(nl: int, **fields) -> np.ndarray:
    """Host table (LISTENER_DTYPE, 64-byte items), LISTENING, the reference's defaults (receive window 0xFFFF, window
    scale 0, advertised MSS 1450, 5 retries of 3 s, ttl 255); scalars or per-listener arrays override."""
    t = np.zeros(nl, LISTENER_DTYPE)
    t["state"] = N.DK_TCP_LSN_LISTENING
    t["receive_window_size"], t["advertised_mss"] = 0xFFFF, 1450
    t["handshake_retries"], t["handshake_timeout_ns"] = 5, 3_000_000_000
    t["ip_word"] = 0x00FF0000
    for k, v in fields.items():
        t[k] = np.asarray(v).astype(LISTENER_DTYPE.fields[k][0])
    return t


def lsn_of_flow(nflows: int, listeners: np.ndarray) -> np.ndarray:
    """The flow_id -> listener row map from the rows' flow_id field; NONE for every other flow."""
    m = np.full(max(nflows, 1), NONE, np.uint32)
    m[listeners["flow_id"]] = np.arange(len(listeners), dtype=np.uint32)
    return m[:nflows] if nflows else m[:0]


def to_device(a: np.ndarray, device: int = 0):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", device))


def listeners_to_host(dev) -> np.ndarray:
    return dev.cpu().numpy().view(LISTENER_DTYPE).copy()


def key(listener: int, remote_ip: int, remote_port: int) -> int:
    return (listener & 0xFFFF) << 48 | (remote_ip & 0xFFFFFFFF) << 16 | (remote_port & 0xFFFF)


def key_fields(k: int) -> tuple:
    return int(k) >> 48, (int(k) >> 16) & 0xFFFFFFFF, int(k) & 0xFFFF


def home(cap: int, k: int) -> int:
    """The slot a key's probe walk starts at (dk_tcp_listen_home): pure host code."""
    return int(N.load_library().dk_tcp_listen_home(cap, k))


class ListenTable:
    """dk_tcp_listen_table: `cap` slots (a power of two) on `device`, all FREE."""

    def __init__(self, cap: int, device: int = 0):
        self.lib = N.load_library()
        self.cap, self.device = cap, device
        h = ctypes.c_void_p()
        _check(self.lib.dk_tcp_listen_table_create(device, cap, ctypes.byref(h)), "dk_tcp_listen_table_create")
        self._t = h

    def close(self) -> None:
        if getattr(self, "_t", None):
            self.lib.dk_tcp_listen_table_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rows(self) -> np.ndarray:
        """Every slot as a SLOT_DTYPE row (waits for the table's calls)."""
        r = np.zeros(self.cap, SLOT_DTYPE)
        _check(self.lib.dk_tcp_listen_table_read(self._t, r.ctypes.data), "dk_tcp_listen_table_read")
        return r

    def write(self, rows: np.ndarray) -> None:
        r = np.ascontiguousarray(rows, SLOT_DTYPE)
        assert len(r) == self.cap
        _check(self.lib.dk_tcp_listen_table_write(self._t, r.ctypes.data), "dk_tcp_listen_table_write")

    def as_map(self) -> dict:
        """key -> row, for the slots that hold a connection. Slot numbers are not part of the contract."""
        return {int(r["key"]): r for r in self.rows() if r["state"] not in (FREE, TOMBSTONE)}

    def consumed(self) -> int:
        c = ctypes.c_uint64()
        _check(self.lib.dk_tcp_listen_table_stats(self._t, None, ctypes.byref(c)), "dk_tcp_listen_table_stats")
        return c.value


class ListenResults:
    """Device outputs of one dk_tcp_listen_process / _timers call (dk_tcp_lsn_results) for n batch frames, up to
    max_frames replies and max_ready ready records, nl listeners; every array starts as `fill` bytes."""

    def __init__(self, n: int, max_frames: int, max_ready: int, nl: int, device: int = 0, fill: int = 0):
        import torch

        dev = torch.device("cuda", device)
        self.n, self.max_frames, self.max_ready, self.nl = n, max_frames, max_ready, nl
        u8 = lambda k: torch.full((max(k, 4),), fill, dtype=torch.uint8, device=dev)  # noqa: E731
        self.action = u8(n)
        self.slot, self.reply_frame = u8(4 * n), u8(4 * n)
        self.off_out, self.len_out, self.frame_seg = u8(4 * max_frames), u8(2 * max_frames), u8(4 * max_frames)
        self.ready = u8(READY_DTYPE.itemsize * max_ready)
        self.status = u8(4 * nl)
        self.n_frames, self.n_ready = u8(4), u8(4)

    def c_struct(self) -> N.DkTcpLsnResults:
        return N.DkTcpLsnResults(*[_ptr(getattr(self, k)) for k in N.TCP_LSN_RESULT_FIELDS])

    def raw(self) -> dict:
        """Every array whole, as bytes (for canary comparisons)."""
        return {k: getattr(self, k).cpu().numpy().copy() for k in N.TCP_LSN_RESULT_FIELDS}

    def to_numpy(self) -> dict:
        r = self.raw()
        u32 = lambda k, m: r[k][:4 * m].view(np.uint32)  # noqa: E731
        return {"action": r["action"][:self.n], "slot": u32("slot", self.n), "reply_frame": u32("reply_frame", self.n),
                "off_out": u32("off_out", self.max_frames), "len_out": r["len_out"][:2 * self.max_frames].view(np.uint16),
                "frame_seg": u32("frame_seg", self.max_frames),
                "ready": r["ready"][:READY_DTYPE.itemsize * self.max_ready].view(READY_DTYPE),
                "status": u32("status", self.nl), "n_frames": int(u32("n_frames", 1)[0]),
                "n_ready": int(u32("n_ready", 1)[0])}


def _stream(stream, device):
    import torch

    return stream if stream is not None else torch.cuda.current_stream(device)


def listen_process(table: ListenTable, rx: RxResults, listeners, lsn_map, links, now_ns: int, out, res: ListenResults,
                   *, slot_stride: int, frame_lead: int = 0, flags: int = 0, backlog_sum: Optional[int] = None,
                   link=None, n: Optional[int] = None, out_bytes=None, max_frames=None, max_ready=None,
                   stream=None) -> None:
    """dk_tcp_listen_process: `rx` are the results of the batch's receive_batch call (tcp_fields and tcp_opts on),
    listeners a uint8 device tensor of LISTENER_DTYPE rows (updated in place), lsn_map the int32 / uint32 device map
    flow_id -> listener row. backlog_sum defaults to the rows' sum (read back from the device, on `stream`: pass it to
    stay asynchronous). Everything the caller passes in, `res` included, must be ready on `stream` (default: the current
    stream): tensors made or filled on another stream need that stream waited for before the call. The same holds for
    listen_timers."""
    import torch

    nl = listeners.numel() // LISTENER_DTYPE.itemsize
    s = _stream(stream, table.device)
    if backlog_sum is None:
        with torch.cuda.stream(s):  # behind the calls that update the rows, which run on this stream
            backlog_sum = int(listeners_to_host(listeners)["max_backlog"].astype(np.uint64).sum())
    r, o = rx.c_struct(), res.c_struct()
    lay = N.DkTcpTxLayout(slot_stride, frame_lead)
    _check(table.lib.dk_tcp_listen_process(
        table._t, ctypes.byref(r), rx.n if n is None else n, _ptr(listeners), nl, backlog_sum, _ptr(lsn_map),
        lsn_map.numel(), _ptr(link), _ptr(links), links.numel() // N.TX_LINK_DTYPE.itemsize, now_ns, _ptr(out),
        out.numel() if out_bytes is None else out_bytes, ctypes.byref(lay),
        res.max_frames if max_frames is None else max_frames, res.max_ready if max_ready is None else max_ready, flags,
        ctypes.byref(o), ctypes.c_void_p(s.cuda_stream)), "dk_tcp_listen_process")


def listen_timers(table: ListenTable, listeners, links, now_ns: int, out, res: ListenResults, *, slot_stride: int,
                  frame_lead: int = 0, flags: int = 0, backlog_sum: int = 0, out_bytes=None, max_frames=None,
                  max_ready=None, stream=None) -> None:
    """dk_tcp_listen_timers: the handshake timeout over every slot of the table."""
    nl = listeners.numel() // LISTENER_DTYPE.itemsize
    s = _stream(stream, table.device)
    o = res.c_struct()
    lay = N.DkTcpTxLayout(slot_stride, frame_lead)
    _check(table.lib.dk_tcp_listen_timers(
        table._t, _ptr(listeners), nl, backlog_sum, _ptr(links), links.numel() // N.TX_LINK_DTYPE.itemsize, now_ns,
        _ptr(out), out.numel() if out_bytes is None else out_bytes, ctypes.byref(lay),
        res.max_frames if max_frames is None else max_frames, res.max_ready if max_ready is None else max_ready, flags,
        ctypes.byref(o), ctypes.c_void_p(s.cuda_stream)), "dk_tcp_listen_timers")


def listen_release(table: ListenTable, listeners, keys, stream=None) -> np.ndarray:
    """dk_tcp_listen_release of `keys` (an iterable of key words); returns found[] (waits for the call). The keys are
    uploaded and found[] is made, filled and read back on `stream` (default: the current stream), the stream the call
    runs on; `listeners` must be ready on it."""
    import torch

    k = np.asarray(list(keys), np.uint64)
    dev = torch.device("cuda", table.device)
    nl = listeners.numel() // LISTENER_DTYPE.itemsize
    s = _stream(stream, table.device)
    with torch.cuda.stream(s):
        kd = torch.from_numpy(k.view(np.int64).copy()).to(dev)
        found = torch.full((max(len(k), 1),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        _check(table.lib.dk_tcp_listen_release(table._t, _ptr(listeners), nl, _ptr(kd), len(k), _ptr(found),
                                               ctypes.c_void_p(s.cuda_stream)), "dk_tcp_listen_release")
        return found.cpu().numpy().view(np.uint32)[:len(k)]


def conn_rows_from_ready(rec, listener_row, *, buffer_size: Optional[int] = None, link: Optional[int] = None):
    """The dk_tcp_conn (CONN_DTYPE) and dk_tcp_tx_conn (TX_CONN_DTYPE) rows of the connection a successful ready
    record describes, as EstablishedSocket::new sets them up: RCV.NXT = reader_next = rcv_nxt, SND.UNA = SND.NXT =
    snd_nxt, the send window = remote_window, the receive buffer = local_window unless given."""
    assert int(rec["err"]) == 0
    rx = np.zeros(1, N.CONN_DTYPE)
    rx["state"] = N.DK_TCP_ESTABLISHED
    rx["receive_next"] = rx["reader_next"] = rec["rcv_nxt"]
    rx["buffer_size"] = int(rec["local_window"]) if buffer_size is None else buffer_size
    rx["send_next"] = rec["snd_nxt"]
    tx = np.zeros(1, N.TX_CONN_DTYPE)
    tx["state"] = N.DK_TCP_ESTABLISHED
    tx["snd_una"] = tx["snd_nxt"] = rec["snd_nxt"]
    tx["snd_wnd"], tx["cwnd"], tx["mss"] = rec["remote_window"], 0xFFFFFFFF, rec["mss"]
    tx["rcv_nxt"], tx["rcv_wscale"] = rec["rcv_nxt"], rec["local_wscale"]
    tx["local_ip"], tx["remote_ip"] = listener_row["local_ip"], rec["remote_ip"]
    tx["ports"] = int(listener_row["local_port"]) | int(rec["remote_port"]) << 16
    tx["ip_word"] = listener_row["ip_word"]
    tx["link"] = listener_row["link"] if link is None else link
    tx["rcv_wnd_hdr"] = min(int(rx["buffer_size"][0]) >> int(rec["local_wscale"]), 0xFFFF)
    return rx, tx
