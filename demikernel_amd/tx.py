"""Host-side mirror of the send chain's header serialization, over the C ABI (include/dk_rx.h, dk_tx_serialize).

The reference (Rust, src/rust/inetstack/protocols/) prepends the headers of one segment at a time:
    TcpHeader::serialize_and_attach / UdpHeader::serialize_and_attach  (layer4/tcp/header.rs:330-405,
                                                                          layer4/udp/header.rs:97-130)
    -> Ipv4Header::serialize_and_attach   (layer3/ipv4/header.rs:229-266, called from layer3/mod.rs:151-160)
    -> Ethernet2Header::serialize_and_attach  (layer2/ethernet2/header.rs:68-73, called from layer2/mod.rs:85-96)
`tx_serialize` does that for a whole batch on one MI355X: the headers are written into the headroom in front of each
payload of an HBM (or mapped pinned) blob, and the returned FrameBatch describes the finished frames, ready for a NIC
ring or for RxEngine.receive_batch (loopback).

The descriptor fields use dk_rx_results' packing, so the arrays a receive call produced can be passed back unchanged
(`TxSegments.from_rx_results`). torch only owns device memory and names the stream.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native as N
from .rx import FrameBatch, RxResults, _check, _ptr

_REQUIRED = ["payload_off", "payload_len", "meta", "src_ip", "dst_ip", "ports"]


def tx_links(pairs) -> np.ndarray:
    """[(dst_mac, src_mac), ...] (6 bytes each) -> TX_LINK_DTYPE array, the `links` argument of tx_serialize."""
    a = np.zeros(len(pairs), N.TX_LINK_DTYPE)
    for i, (dst, src) in enumerate(pairs):
        a["dst_mac"][i] = np.frombuffer(bytes(dst), np.uint8)
        a["src_mac"][i] = np.frombuffer(bytes(src), np.uint8)
    return a


def tx_header_bytes(ip_protocol: int, opts: Optional[np.ndarray] = None) -> int:
    """dk_tx_header_bytes: header bytes in front of the payload for a protocol and one TCP_OPTS_DTYPE record (None: no
    options); 0 if it cannot be serialized."""
    lib = N.load_library()
    if opts is None:
        return lib.dk_tx_header_bytes(ip_protocol, None)
    rec = np.ascontiguousarray(opts, N.TCP_OPTS_DTYPE).reshape(-1)[:1]
    return lib.dk_tx_header_bytes(ip_protocol, rec.ctypes.data)


def ip_word(ident, ttl, dscp_ecn=0) -> np.ndarray:
    """dk_tx_segs.ip_word: identification | ttl << 16 | (dscp << 2 | ecn) << 24."""
    return (np.asarray(ident, np.uint32) & 0xFFFF) | (np.asarray(ttl, np.uint32) & 0xFF) << 16 \
        | (np.asarray(dscp_ecn, np.uint32) & 0xFF) << 24


class TxSegments:
    """The segments of one dk_tx_serialize call (struct dk_tx_segs): device tensors, owned (from_numpy) or borrowed
    (from_rx_results). int32 / int16 / uint8 storage reinterpreted as the ABI's u32 / u16 / dk_tcp_opts."""

    def __init__(self, n: int, arrays: dict):
        import torch

        for k in _REQUIRED:
            assert arrays.get(k) is not None, f"dk_tx_segs.{k} is required"
        for k, t in arrays.items():
            assert k in N.TX_SEG_FIELDS, k
            if t is None:
                continue
            want = torch.uint8 if k == "tcp_opts" else torch.int16 if k == "payload_len" else torch.int32
            size = n * N.TCP_OPTS_DTYPE.itemsize if k == "tcp_opts" else n
            assert t.dtype == want and t.numel() >= size and t.is_contiguous(), k
        self.n = n
        self.t = {k: v for k, v in arrays.items() if v is not None}

    @staticmethod
    def _upload(name: str, a, dev):
        import torch

        if a is None or hasattr(a, "data_ptr"):
            return a
        if name == "tcp_opts":
            h = np.ascontiguousarray(a, N.TCP_OPTS_DTYPE).view(np.uint8).reshape(-1)
            if h.size == 0:
                h = np.zeros(N.TCP_OPTS_DTYPE.itemsize, np.uint8)
        elif name == "payload_len":
            h = np.ascontiguousarray(a, np.uint16).view(np.int16)
        else:
            h = np.ascontiguousarray(a, np.uint32).view(np.int32)
        return torch.from_numpy(h.copy()).to(dev)

    @classmethod
    def from_numpy(cls, payload_off, payload_len, meta, src_ip, dst_ip, ports, *, tcp_seq=None, tcp_ack=None,
                   tcp_win=None, tcp_opts=None, ip_word=None, link=None, device: int = 0) -> "TxSegments":
        import torch

        dev = torch.device("cuda", device)
        given = dict(payload_off=payload_off, payload_len=payload_len, meta=meta, src_ip=src_ip, dst_ip=dst_ip,
                     ports=ports, tcp_seq=tcp_seq, tcp_ack=tcp_ack, tcp_win=tcp_win, tcp_opts=tcp_opts,
                     ip_word=ip_word, link=link)
        return cls(len(payload_off), {k: cls._upload(k, v, dev) for k, v in given.items()})

    @classmethod
    def from_rx_results(cls, results, payload_off, payload_len, *, ip_word=None, link=None,
                        device: int = 0) -> "TxSegments":
        """Segments whose header fields are a receive call's results, passed back unchanged: `results` is an RxResults
        (its device arrays are borrowed, not copied) or a dict of arrays in the same packing. payload_off is the
        payload's byte offset in the blob that is serialized into (for the blob that was received: the frame's offset
        plus the low half of results' `payload`), payload_len its length."""
        import torch

        src = results.t if isinstance(results, RxResults) else results
        ref = next((v for v in src.values() if hasattr(v, "data_ptr")), None)  # a torch tensor among them
        dev = ref.device if ref is not None else torch.device("cuda", device)
        arrays = {k: cls._upload(k, src.get(k), dev)
                  for k in ("meta", "src_ip", "dst_ip", "ports", "tcp_seq", "tcp_ack", "tcp_win", "tcp_opts")}
        arrays.update(payload_off=cls._upload("payload_off", payload_off, dev),
                      payload_len=cls._upload("payload_len", payload_len, dev),
                      ip_word=cls._upload("ip_word", ip_word, dev), link=cls._upload("link", link, dev))
        return cls(arrays["payload_off"].numel(), arrays)

    def c_struct(self, flags: int = 0) -> N.DkTxSegs:
        return N.DkTxSegs(*[_ptr(self.t.get(name)) for name in N.TX_SEG_FIELDS], self.n, flags)


def tx_serialize(blob, segs: TxSegments, links, *, offload_tcp: bool = False, offload_udp: bool = False, stream=None,
                 status: bool = True, out=None) -> FrameBatch:
    """dk_tx_serialize: build the Ethernet / IPv4 / TCP or UDP headers of every segment in front of its payload in
    `blob` (a uint8 device or pinned tensor), asynchronously on `stream` (default: the current stream). `links` is a
    TX_LINK_DTYPE array (tx_links) or a device uint8 tensor holding such records. Returns a FrameBatch over the same
    blob whose off / len are the call's outputs (0 / 0 for a segment that failed), with the per-segment status tensor
    (int32, N.DK_TX_*) as its `status` attribute (None with status=False). out: (off, len, status or None) device
    tensors of n entries (int32, int16, int32) to write into instead of new ones — a send loop's preallocated outputs.
    The call queues nothing but its one kernel, and that on `stream`: the outputs are allocated uninitialised (the
    kernel writes every entry), so nothing on torch's current stream can land on them after the kernel."""
    import torch

    dev = segs.t["payload_off"].device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    if not hasattr(links, "data_ptr"):
        h = np.ascontiguousarray(links, N.TX_LINK_DTYPE).view(np.uint8).reshape(-1)
        links = torch.from_numpy(h.copy()).to(dev)
    nlinks = links.numel() // N.TX_LINK_DTYPE.itemsize
    n = segs.n
    if out is not None:
        off, lens, st = out
        assert off.dtype == torch.int32 and lens.dtype == torch.int16 and off.numel() == lens.numel() == n
        assert st is None or (st.dtype == torch.int32 and st.numel() == n)
    else:
        off = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
        lens = torch.empty(max(n, 1), dtype=torch.int16, device=dev)[:n]
        st = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n] if status else None
        for t in (off, lens, st):  # allocated from the current stream's pool, written on `s`
            if t is not None and t.is_cuda:
                t.record_stream(s)
    flags = (N.DK_TX_OFFLOAD_TCP if offload_tcp else 0) | (N.DK_TX_OFFLOAD_UDP if offload_udp else 0)
    cs = segs.c_struct(flags)
    _check(N.load_library().dk_tx_serialize(_ptr(blob), blob.numel(), ctypes.byref(cs), _ptr(links), nlinks,
                                            _ptr(off), _ptr(lens), _ptr(st), ctypes.c_void_p(s.cuda_stream)),
           "dk_tx_serialize")
    batch = FrameBatch(blob, off, lens)
    batch.status = st
    batch.links = links  # read by the queued kernel: kept alive with the batch
    batch.segs = segs
    return batch


def tx_serialize_grid(grid: int = -1) -> None:
    """Diagnostics (dk_diag.h): cap dk_tx_serialize's grid at `grid` workgroups for the process (<= 0: the rule)."""
    _check(N.load_library().dk_diag_tx_serialize_set_grid(grid), "dk_diag_tx_serialize_set_grid")
