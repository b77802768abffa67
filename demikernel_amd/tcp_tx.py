"""TCP send segmentation on the GPU (include/dk_tcp.h, dk_tcp_tx_segment).

What a loop of Sender::send_segment (tcp/established/sender.rs:124-208) does to the buffers an application pushed,
for every connection of a batch at once: each buffer is cut into segments of min(send window - in flight, MSS,
cwnd - in flight) bytes, PSH on the piece that ends a buffer, a zero-length buffer becomes the FIN, SND.NXT advances,
and every piece is copied into a frame slot behind the 54 header bytes ControlBlock::tcp_header and the serialize chain
give it, the TCP checksum summed while the payload is copied. The send side of the connections is a device array of
struct dk_tcp_tx_conn (TX_CONN_DTYPE), updated in place; the ack number and window of the outgoing headers come from it
or straight from the dk_tcp_conn table TcpReceiver.process keeps.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native as N
from .rx import FrameBatch, _check, _ptr

TX_CONN_DTYPE = N.TX_CONN_DTYPE
STATUSES = N.TCP_TX_STATUSES
SENT, PARTIAL, UNSENT, CLOSED, E_CONN, NO_ROOM = range(6)


def tx_conn_table(nconns: int, *, snd_nxt=0, snd_una=None, snd_wnd=65535, cwnd=0xFFFFFFFF, mss=1460, rcv_nxt=0,
                  rcv_wnd_hdr=65535, rcv_wscale=0, local_ip=0, remote_ip=0, ports=0, ip_word=0x00FF0000, link=0,
                  state=N.DK_TCP_ESTABLISHED) -> np.ndarray:
    """Host table of send sides (TX_CONN_DTYPE): established, nothing in flight unless snd_una is given, congestion
    control None (cwnd = u32::MAX), Ipv4Header::new's identification / ttl / dscp. Scalars or per-connection arrays."""
    t = np.zeros(nconns, TX_CONN_DTYPE)
    u32 = lambda v: np.asarray(v, np.int64).astype(np.uint32)  # noqa: E731
    t["state"] = state
    t["snd_nxt"] = u32(snd_nxt)
    t["snd_una"] = t["snd_nxt"] if snd_una is None else u32(snd_una)
    for k, v in (("snd_wnd", snd_wnd), ("cwnd", cwnd), ("mss", mss), ("rcv_nxt", rcv_nxt), ("rcv_wscale", rcv_wscale),
                 ("local_ip", local_ip), ("remote_ip", remote_ip), ("ports", ports), ("ip_word", ip_word),
                 ("link", link)):
        t[k] = u32(v)
    t["rcv_wnd_hdr"] = rcv_wnd_hdr
    return t


def frame_bound(lens, mss: int) -> int:
    """dk_tcp_tx_frame_bound: the most frames a push list of these lengths can need, sum of max(1, ceil(len / mss))."""
    a = np.ascontiguousarray(lens, np.uint32)
    return int(N.load_library().dk_tcp_tx_frame_bound(a.ctypes.data, a.size, mss))


class TcpTxResults:
    """Device outputs of one dk_tcp_tx_segment call (dk_tcp_tx_results) for up to max_frames frames and nbufs buffers."""

    def __init__(self, max_frames: int, nbufs: int, device: int = 0, frame_buf: bool = True):
        import torch

        dev = torch.device("cuda", device)
        self.max_frames, self.nbufs = max_frames, nbufs
        i32 = lambda k: torch.zeros(max(k, 1), dtype=torch.int32, device=dev)  # noqa: E731
        self.off_out = i32(max_frames)
        self.len_out = torch.zeros(max(max_frames, 1), dtype=torch.int16, device=dev)
        self.frame_buf = i32(max_frames) if frame_buf else None
        self.sent, self.first_frame, self.frame_count, self.status = i32(nbufs), i32(nbufs), i32(nbufs), i32(nbufs)
        self.n_frames = i32(1)

    def c_struct(self) -> N.DkTcpTxResults:
        return N.DkTcpTxResults(*[_ptr(getattr(self, k)) for k in N.TCP_TX_RESULT_FIELDS])

    def to_numpy(self) -> dict:
        """Host copies (synchronises). Per-frame arrays are cut to the frames written (none when the call ran out of
        room); n_frames is the plan's need."""
        need = int(self.n_frames.cpu().numpy().view(np.uint32)[0])
        st = self.status.cpu().numpy().view(np.uint32)[:self.nbufs]
        wrote = need if need <= self.max_frames and not (st == NO_ROOM).any() else 0
        h = {"n_frames": need, "frames_written": wrote, "status": st,
             "off_out": self.off_out.cpu().numpy().view(np.uint32)[:wrote],
             "len_out": self.len_out.cpu().numpy().view(np.uint16)[:wrote]}
        if self.frame_buf is not None:
            h["frame_buf"] = self.frame_buf.cpu().numpy().view(np.uint32)[:wrote]
        for k in ("sent", "first_frame", "frame_count"):
            h[k] = getattr(self, k).cpu().numpy().view(np.uint32)[:self.nbufs]
        return h


class PushList:
    """The pushed buffers of one call (dk_tcp_tx_push): int32 device tensors conn (non-decreasing), off, len."""

    def __init__(self, conn, off, lens):
        import torch

        for t in (conn, off, lens):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == conn.numel()
        self.conn, self.off, self.len = conn, off, lens
        self.n = conn.numel()

    @classmethod
    def from_numpy(cls, conn, off, lens, device: int = 0) -> "PushList":
        import torch

        dev = torch.device("cuda", device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).to(dev)  # noqa: E731
        return cls(up(conn), up(off), up(lens))

    def c_struct(self) -> N.DkTcpTxPush:
        return N.DkTcpTxPush(_ptr(self.conn), _ptr(self.off), _ptr(self.len))


class TcpSender:
    """Per-GPU TCP send segmentation over a device table of send sides (the Sender halves of the ControlBlocks)."""

    def __init__(self, device: int = 0, lib_path: str | None = None):
        self.lib = N.load_library(lib_path) if lib_path else N.load_library()
        self.device = device
        h = ctypes.c_void_p()
        _check(self.lib.dk_tcp_tx_ctx_create(device, ctypes.byref(h)), "dk_tcp_tx_ctx_create")
        self._ctx = h

    def close(self) -> None:
        if self._ctx:
            self.lib.dk_tcp_tx_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def conns_to_device(self, table: np.ndarray):
        import torch

        t = np.ascontiguousarray(table, TX_CONN_DTYPE)
        return torch.from_numpy(t.view(np.uint8).copy()).to(torch.device("cuda", self.device))

    @staticmethod
    def conns_to_host(dev) -> np.ndarray:
        return dev.cpu().numpy().view(TX_CONN_DTYPE).copy()

    def segment(self, src, push: PushList, tx_conns, links, out, res: TcpTxResults, *, slot_stride: int = 1536,
                frame_lead: int = 0, rx_conns=None, offload_tcp: bool = False, stream=None,
                src_bytes: Optional[int] = None, out_bytes: Optional[int] = None,
                max_frames: Optional[int] = None) -> None:
        """dk_tcp_tx_segment: cut `push` (ranges of the uint8 device tensor `src`) into frames in `out` (uint8 device
        tensor; frame f at f * slot_stride + frame_lead), asynchronously on `stream` (default: the current stream).
        tx_conns: uint8 device tensor of TX_CONN_DTYPE records, updated in place; rx_conns: optionally the CONN_DTYPE
        table of the same connections (ack number and window are then read from it); links: a device uint8 tensor of
        TX_LINK_DTYPE records. Results land in `res`."""
        import torch

        assert tx_conns.dtype == torch.uint8 and tx_conns.numel() % TX_CONN_DTYPE.itemsize == 0
        nconns = tx_conns.numel() // TX_CONN_DTYPE.itemsize
        assert rx_conns is None or rx_conns.numel() == nconns * N.CONN_DTYPE.itemsize
        assert res.nbufs >= push.n
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        p, r = push.c_struct(), res.c_struct()
        lay = N.DkTcpTxLayout(slot_stride, frame_lead)
        _check(self.lib.dk_tcp_tx_segment(
            self._ctx, _ptr(src), src.numel() if src_bytes is None else src_bytes, ctypes.byref(p), push.n,
            _ptr(tx_conns), nconns, _ptr(rx_conns), _ptr(links), links.numel() // N.TX_LINK_DTYPE.itemsize, _ptr(out),
            out.numel() if out_bytes is None else out_bytes, ctypes.byref(lay),
            res.max_frames if max_frames is None else max_frames, N.DK_TX_OFFLOAD_TCP if offload_tcp else 0,
            ctypes.byref(r), ctypes.c_void_p(s.cuda_stream)), "dk_tcp_tx_segment")

    def segment_batch(self, src, push: PushList, tx_conns, links, out, res: TcpTxResults, **kw) -> FrameBatch:
        """segment(), then the frames it wrote as a FrameBatch over `out`, ready for RxEngine.receive_batch or a NIC
        ring. Reads n_frames back, so it waits for the call; an empty batch when the call ran out of room (res then
        says how many frames it needs)."""
        import torch

        self.segment(src, push, tx_conns, links, out, res, **kw)
        stream = kw.get("stream")
        (stream if stream is not None else torch.cuda.current_stream(self.device)).synchronize()
        need = int(res.n_frames.cpu().numpy().view(np.uint32)[0])
        cap = res.max_frames if kw.get("max_frames") is None else kw["max_frames"]
        ob = out.numel() if kw.get("out_bytes") is None else kw["out_bytes"]
        n = need if need <= cap and need * kw.get("slot_stride", 1536) <= ob else 0
        batch = FrameBatch(out, res.off_out[:n], res.len_out[:n])
        batch.results = res
        return batch


def tcp_tx_grid(grid: int = -1) -> None:
    """Diagnostics (dk_diag.h): cap the emit kernel's grid at `grid` workgroups for the process (<= 0: the rule)."""
    _check(N.load_library().dk_diag_tcp_tx_set_grid(grid), "dk_diag_tcp_tx_set_grid")
