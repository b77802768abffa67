"""dk_tcp_cc_send on the MI355X against tests/tcp_cc_reference.py, around a real dk_tcp_tx_segment call: both phases,
connections that get 0, 1 and 5 frames, a limited-transmit increase of 2 mss against a first frame smaller than it, an
end-of-send marker, a None row, failing rows, and a segmentation call that ran out of room. Every table is compared
whole after each phase."""
import errno

import numpy as np
import pytest

import tcp_cc_reference as R
import tx_segment_reference as M
from demikernel_amd import _native as N
from demikernel_amd import synth
from demikernel_amd.rx import Fail
from demikernel_amd.tcp_ack import ack_conn_table
from demikernel_amd.tcp_cc import AFTER_SEND, BEFORE_SEND, cc_conn_table, cc_send, cc_to_device, cc_to_host
from demikernel_amd.tcp_tx import PushList, TcpSender, TcpTxResults

pytestmark = pytest.mark.gpu
NOW = 40 * 10**9
MSS, NC = 1000, 10
CANARY = 0x5A5A5A5A
# connection -> the buffers pushed on it
PUSHES = {1: [700], 2: [4700], 3: [700, 1000], 4: [900], 5: [1000], 6: [2500], 7: [100], 8: [300, 0], 9: [800]}


@pytest.fixture(scope="module")
def sender():
    s = TcpSender(0)
    yield s
    s.close()


def tables():
    flows = synth.make_flows(NC, passive=False)
    snd = np.arange(NC, dtype=np.int64) * 1_000_003 + 0xFFFFF000  # some wrap
    tx = M.conns_toward(flows, snd_nxt=snd, snd_wnd=1 << 20, mss=MSS, cwnd=0x01020304, link=0)
    ak = ack_conn_table(NC)
    ak["rto"] = 0.25
    cc = cc_conn_table(NC, mss=MSS, now_ns=NOW - 10**8)  # sent 0.1 s ago, rtt_at_last_send 1 s: not idle
    cc["ltci"] = 2 * MSS
    tx["snd_una"][4] -= 500                      # 500 bytes already in flight
    cc["cwnd"][5], cc["last_send_ns"][5] = 9 * MSS, NOW - 10**9 - 1   # idle: restarts at initial_cwnd, no increase
    cc[6] = cc_conn_table(1, mss=MSS, cubic=False)[0]                 # None
    tx["cwnd"][6] = 0xFFFFFFFF
    tx["state"][7] = N.DK_TCP_CLOSED
    return tx, ak, cc


def run(sender, max_frames=32, rto9=float("nan")):
    import torch

    tx, ak, cc = tables()
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
    d_tx, d_ak, d_cc, d_links = up(tx), up(ak), cc_to_device(cc), up(M.links_table())
    status = torch.full((NC,), CANARY, dtype=torch.int32, device=dev)
    # before
    cc_send(sender, BEFORE_SEND, d_tx, d_ak, d_cc, NOW, status)
    torch.cuda.synchronize()
    e_tx, e_cc = tx.copy(), cc.copy()
    e_st = R.cc_send_before(e_tx, e_cc, NOW)
    g_tx, g_cc = d_tx.cpu().numpy().view(N.TX_CONN_DTYPE).copy(), cc_to_host(d_cc)
    assert np.array_equal(status.cpu().numpy().view(np.uint32), e_st) and e_st.tolist() == [0] * 7 + [R.E_STATE, 0, 0]
    assert g_tx.tobytes() == e_tx.tobytes() and g_cc.tobytes() == e_cc.tobytes()
    assert g_tx["cwnd"].tolist() == [6000] * 5 + [4000, 0xFFFFFFFF, 0x01020304, 6000, 6000]
    assert (g_cc["cwnd"][5], g_cc["ltci"][5]) == (4 * MSS, 0)
    # the segmentation call between the hooks
    conn = [c for c, lens in PUSHES.items() for _ in lens]
    lens = [ln for lens_ in PUSHES.values() for ln in lens_]
    src, pconn, poff, plen = M.pack_push(conn, lens)
    push = PushList.from_numpy(pconn, poff, plen)
    res = TcpTxResults(32, len(lens))
    d_out = torch.zeros(32 * 1100, dtype=torch.uint8, device=dev)
    sender.segment(torch.from_numpy(src).to(dev), push, d_tx, d_links, d_out, res, slot_stride=1100, max_frames=max_frames)
    torch.cuda.synchronize()
    h = res.to_numpy()
    sent_tx = d_tx.cpu().numpy().view(N.TX_CONN_DTYPE).copy()
    # after; connection 9's rto turns invalid first
    ak["rto"][9] = rto9
    d_ak = up(ak)
    status.fill_(CANARY)
    cc_send(sender, AFTER_SEND, d_tx, d_ak, d_cc, NOW + 5, status, push=push, res=res)
    torch.cuda.synchronize()
    frames = [[] for _ in range(NC)]
    for f in range(h["frames_written"]):
        bytes_ = int(h["len_out"][f]) - 54
        frames[conn[int(h["frame_buf"][f])]].append(bytes_ if bytes_ else 1)
    e_tx, e_cc2 = sent_tx.copy(), e_cc.copy()
    e_st = R.cc_send_after(e_tx, ak, e_cc2, NOW + 5, frames)
    g_tx, g_cc = d_tx.cpu().numpy().view(N.TX_CONN_DTYPE).copy(), cc_to_host(d_cc)
    assert np.array_equal(status.cpu().numpy().view(np.uint32), e_st)
    rows = [c for c in range(NC) if g_cc[c].tobytes() != e_cc2[c].tobytes() or g_tx[c].tobytes() != e_tx[c].tobytes()]
    assert not rows, (rows, g_cc[rows], e_cc2[rows])
    assert d_ak.cpu().numpy().tobytes() == ak.tobytes()
    return h, frames, e_cc, g_cc, g_tx, e_st


def test_both_phases(sender):
    h, frames, before, cc, tx, st = run(sender)
    assert [len(f) for f in frames] == [0, 1, 5, 2, 1, 1, 3, 0, 2, 1]
    assert frames[2] == [1000, 1000, 1000, 1000, 700] and frames[3] == [700, 1000] and frames[8] == [300, 1]
    assert st.tolist() == [0] * 7 + [R.E_STATE, 0, R.E_RTO]
    # on_send is given the bytes in flight before each frame (sender.rs:177): 2 mss of increase become
    #   1: 0 in flight                       -> 2,000      2: 0, 1,000, 2,000, ...  -> 2,000, 1,000, 0
    #   3: 0, then 700 (the first frame)     -> 1,300      4: 500 already in flight -> 1,500
    #   8: 0, then 300                       -> 1,700
    assert cc["ltci"].tolist()[:5] == [2000, 2000, 0, 1300, 1500] and cc["ltci"][8] == 1700
    sent = np.array([len(f) > 0 for f in frames])
    ok = sent & (st == 0) & (before["flags"] & R.CUBIC != 0)
    assert (cc["last_send_ns"][ok] == NOW + 5).all() and (cc["rtt_at_last_send_ns"][ok] == 250_000_000).all()
    assert cc[[0, 6, 7, 9]].tobytes() == before[[0, 6, 7, 9]].tobytes()  # no frame, None, E_STATE, E_RTO: untouched
    assert tx["cwnd"].tolist() == [6000, 6000, 4000, 5300, 5500, 4000, 0xFFFFFFFF, 0x01020304, 5700, 6000]


def test_a_call_out_of_room_changes_nothing(sender):
    h, frames, before, cc, tx, st = run(sender, max_frames=3, rto9=0.25)
    assert h["frames_written"] == 0 and h["n_frames"] > 3 and (h["status"] == N.DK_TCP_TX_NO_ROOM).sum() >= 8
    assert cc.tobytes() == before.tobytes() and st.tolist() == [0] * 7 + [R.E_STATE, 0, 0]


def test_argument_errors(sender):
    import torch

    tx, ak, cc = tables()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()  # noqa: E731
    d_tx, d_ak, d_cc = up(tx), up(ak), cc_to_device(cc)
    status = torch.zeros(NC, dtype=torch.int32, device=d_tx.device)
    for phase in (2, 77):
        with pytest.raises(Fail) as e:
            cc_send(sender, phase, d_tx, d_ak, d_cc, NOW, status, push=PushList.from_numpy([0], [0], [1]),
                    res=TcpTxResults(1, 1))
        assert e.value.errno == errno.EINVAL
    torch.cuda.synchronize()
    assert cc_to_host(d_cc).tobytes() == cc.tobytes()
