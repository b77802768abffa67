"""The control-plane families' promise "calls on one table / one pool are serialised; asynchronous on the caller's
stream", tested so that a missing order shows.

Every chain runs on two streams A and B that really run side by side (ctl_calls.stream_pair) and puts about 100 ms of
sleep on A first (ctl_calls.delayed), so the first call is still pending when the second is queued on B: without the
library's own ordering B's call runs first. Uploads and result fills are done before, on the current stream, and both
streams wait for them. The calls are then issued with no host wait between them, and right after each test asserts
that the delay's event has not completed. The harness comparisons (bit-exact, canary tails, the whole blob, the tables
afterwards) run at the end, each call against the model in issue order. Each chain also checks on the CPU, with the
model alone, that applying the second call before the first gives another answer than the one asserted.

dk_tcp_listen_release and dk_arp_lookup return host arrays, so their wrappers wait for the call: a chain that ends in
one asserts the pending delay just before it. CallScratch::grow waits on the host for the scratch's last call before it
frees it, so the growth cases assert the pending delay before the growing call and not after it. The scratch of connect
and close is the process's pool: there the growing call grows it when no earlier test of the process needed as much,
which is always so when this module runs alone; a listen or ARP table brings its own scratch and always grows."""
import copy

import numpy as np
import pytest

import arp_cases as AC
import arp_reference as AR
import tcp_close_cases as CLC
import tcp_connect_cases as CC
import tcp_connect_reference as CR
import tcp_listen_cases as LC
import tcp_listen_reference as LR
import test_gpu_arp as GA
import test_gpu_tcp_close as GCL
import test_gpu_tcp_connect as GC
import test_gpu_tcp_listen as GL
from ctl_calls import Call, delayed, stream_pair
from demikernel_amd import _native as N
from demikernel_amd import arp as ARP
from demikernel_amd import ipv4
from demikernel_amd import tcp_close as TCL
from demikernel_amd import tcp_connect as TC
from demikernel_amd import tcp_listen as TL

pytestmark = pytest.mark.gpu

K = 32
BIG = 1 << 20
LARGE = 2049
T0 = 1_000_000


@pytest.fixture
def closing():
    made = []
    yield made.append
    for d in made:
        d.close()


@pytest.fixture
def pair():
    """(A, B): two streams that run side by side, both behind what the current stream has queued when they are used."""
    import torch

    a, b, which = stream_pair()
    print(f"\nstream pair {which} of 8 fresh streams")
    torch.cuda.synchronize()
    return a, b


def ready(*streams):
    """The uploads and fills, queued on the current stream, come before whatever the streams run next."""
    import torch

    for s in streams:
        s.wait_stream(torch.cuda.current_stream())


def finish(*calls):
    return [c.finish() for c in calls]


# ---- the cases --------------------------------------------------------------------------------------------------------------
def listen_device(closing, cap=512, backlog=64):
    flows, L, lsn = LC.server([80, 81], max_backlog=backlog, nonce=[0x1234, 0xCAFEF00D], isn_counter=[5, 0xFFF0])
    d = GL.Device(flows, L, lsn, cap=cap)
    closing(d)
    return d, flows


def listen_chain(d, flows, k, first=0):
    """k SYNs of k remotes, the ACKs that complete their handshakes (every fifth acknowledges a wrong number) and the
    keys of the accepted connections with one that is not in the table."""
    rem = [LC.remote(first + j) for j in range(k)]
    syns = [LC.seg(r, 80 + (j & 1), LR.SYN, seq=1000 * j, options=LC.OPT_MSS_WS0) for j, r in enumerate(rem)]
    m = copy.deepcopy(d.model)
    e = m.process(LC.oracle_rx(syns, flows), d.lsn, T0, LC.LINKS, slot_stride=64, max_frames=BIG, out_bytes=1 << 30, max_ready=BIG)
    assert (e["action"] == TL.SYN_ACCEPTED).all()
    isn = [m.conns[TL.key(j & 1, *r)]["local_isn"] for j, r in enumerate(rem)]
    acks = [LC.seg(r, 80 + (j & 1), LR.ACK, seq=1000 * j + 1, ack=isn[j] + 1 + (j % 5 == 4)) for j, r in enumerate(rem)]
    keys = [TL.key(j & 1, *r) for j, r in enumerate(rem) if j % 5 != 4 and j % 3] + [TL.key(0, *LC.remote(first + 7777))]
    return syns, acks, keys


def connect_device(closing, k, first=0):
    i = np.arange(k)
    flows, rows, cmap = CC.client(k, first=first, handshake_retries=2 + i % 2, link=i % 2, handshake_timeout_ns=1000)
    d = GC.Device(flows, rows, cmap, nonce=0xC0FFEE11, counter=0xFFF0)
    closing(d)
    return d, flows


def connect_answers(d, k, first=0):
    """A SYN+ACK for three rows of four (every eighth is a RST), as connect_start at T0 will have numbered them."""
    m = copy.deepcopy(d.model)
    m.start(list(range(k)), T0, CC.LINKS, slot_stride=64, max_frames=BIG, out_bytes=1 << 40, max_ready=BIG)
    fr = []
    for r in range(k):
        a = int(m.rows[r]["local_isn"]) + 1
        if r % 4 != 3:
            fr.append(CC.seg(first + r, (CR.RST if r % 8 == 5 else CR.SYN) | CR.ACK, seq=77 * r, ack=a, options=CC.OPT_MSS_WS0))
        else:
            fr.append(CC.OTHER[r % len(CC.OTHER)])
    return fr


def close_device(k, seed=31):
    """k IDLE connections ready to be closed: every third has seen the peer's FIN already (LAST-ACK on close)."""
    t = CLC.table([TCL.IDLE] * k, seed=seed)
    t["tx"]["state"] = N.DK_TCP_ESTABLISHED
    t["rx"]["state"] = np.where(np.arange(k) % 3 == 2, N.DK_TCP_CLOSED, N.DK_TCP_ESTABLISHED)
    t["rows"]["linger_ns"] = 1000
    return GCL.Device(t), t


def close_answers(t, rows):
    """The peer's ACK+FIN for the rows in FIN-WAIT-1 after close(), its ACK for those in LAST-ACK; other traffic between."""
    segs = []
    for c in rows:
        segs.append(CLC.seg(t, c, "A" if c % 3 == 2 else "AF"))
        if c % 4 == 1:
            segs.append(None)
    return segs


def arp_device(closing, k, first=0, cap=256, extra_rows=0):
    rows = AC.idle([AC.host(first + 1 + r) for r in range(k + extra_rows)],  # a link belongs to one row's address
                   links=[r if r < 4 else AR.NO_LINK for r in range(k + extra_rows)])
    d = GA.Device(AC.Case(f"chain_{first}", cap=cap, rows=rows, links=AC.links_of(4)))
    closing(d)
    return d


def arp_replies(k, first=0):
    """A reply to us from three hosts of four, a request for us from the fourth."""
    return [(AC.req if r % 4 == 3 else AC.rep)(AC.host(first + 1 + r), AC.ALICE, sha=AC.mac_of(first + r)) for r in range(k)]


def warm_table(d, n):
    """An ARP table's scratch grown to what a process call of n frames needs, by a call that changes nothing: a call
    that grows the scratch waits on the host for the call before it, which the chains must not."""
    import frames as F

    d.process([F.tcp_frame(b"abc")] * n, 1)


def warm_pools(closing):
    """The process's connect and close pools grown past what the chains below need: a call that grows its scratch
    waits on the host for the call before it, which the chains must not."""
    d, flows = connect_device(closing, 4 * K, first=3000)
    d.start(list(range(4 * K)), 5)
    d.process([CC.OTHER[j % 4] for j in range(4 * K)], 6)
    d.timers(7)
    c, t = close_device(4 * K, seed=5)
    c.start(list(range(4 * K)))
    c.process([None] * (4 * K), 8)
    c.timers(9)


# ---- B. a dependent chain per family ------------------------------------------------------------------------------------
def test_listen_chain(closing, pair):
    """listen_process of K SYNs on A, listen_process of their ACKs on B, listen_release of the accepted keys on A. In
    order, the ACKs find their half-open slots and the releases their keys; with B first every ACK meets an empty table
    and is answered with a RST."""
    A, B = pair
    d, flows = listen_device(closing)
    syns, acks, keys = listen_chain(d, flows, K)
    swapped = copy.deepcopy(d.model).process(LC.oracle_rx(acks, flows), d.lsn, T0 + 10, LC.LINKS, slot_stride=64,
                                             max_frames=BIG, out_bytes=1 << 30, max_ready=BIG)
    assert (swapped["action"] == TL.RST_FLAGS).all() and swapped["n_ready"] == 0
    rel = frozenset(keys)
    c1 = Call(d.process_steps(syns, T0, stream=A, state=False, released=rel))
    c2 = Call(d.process_steps(acks, T0 + 10, stream=B, state=False, released=rel))
    ready(A, B)
    ev = delayed(A)
    c1.issue()
    c2.issue()
    assert not ev.query(), "the delay on A ended before the chain was queued: lengthen it"
    found = TL.listen_release(d.table, d.d_L, keys, stream=A)
    (_, e1), (_, e2) = finish(c1, c2)
    assert (e1["action"] == TL.SYN_ACCEPTED).all()
    assert set(int(a) for a in e2["action"]) == {TL.ESTABLISHED, TL.BAD_ACK} and e2["n_ready"] == K and e2["n_frames"] == 0
    want = d.model.release(keys)
    assert [int(x) for x in found] == want == [1] * (len(keys) - 1) + [0]
    d.compare_state()


def test_connect_chain(closing, pair):
    """connect_start on A, connect_process of the SYN+ACKs on B, connect_timers on A past the deadline: established
    rows do not resend. With B first the SYN+ACKs meet IDLE rows, are skipped, and every row resends."""
    A, B = pair
    warm_pools(closing)
    d, flows = connect_device(closing, K)
    fr = connect_answers(d, K)
    m = copy.deepcopy(d.model)
    swapped = m.process(CC.oracle_rx(fr, flows), d.cmap, T0 + 100, CC.LINKS, slot_stride=64, max_frames=BIG,
                        out_bytes=1 << 40, max_ready=BIG)
    assert (swapped["action"] == TC.SKIP).all()
    c1 = Call(d.start_steps(list(range(K)), T0, stream=A, state=False))
    c2 = Call(d.process_steps(fr, T0 + 100, stream=B, state=False))
    c3 = Call(d.timers_steps(T0 + 1000, stream=A, max_frames=K, max_ready=K))
    ready(A, B)
    ev = delayed(A)
    c1.issue()
    c2.issue()
    c3.issue()
    assert not ev.query(), "the delay on A ended before the chain was queued: lengthen it"
    (_, e1), (_, e2), (_, e3) = finish(c1, c2, c3)
    assert e1["n_frames"] == K
    assert set(int(a) for a in e2["action"]) == {TC.SKIP, TC.ESTABLISHED, TC.REFUSED}
    assert e3["frame_seg"] == [r for r in range(K) if r % 4 == 3] and e3["n_ready"] == 0  # only the unanswered rows resend


def test_close_chain(closing, pair):
    """close_start on A, close_process of the peer's ACK+FIN on B, close_timers on A after the linger. With B first the
    segments meet IDLE rows and nothing ever reaches TIME-WAIT."""
    A, B = pair
    warm_pools(closing)
    d, t = close_device(K)
    segs = close_answers(t, range(0, K, 2))
    swapped = copy.deepcopy(d.model).process(CLC.rx_arrays(segs, K), CLC.NOW, CLC.LINKS, slot_stride=64, max_frames=BIG,
                                             out_bytes=1 << 30, max_done=BIG)
    assert (swapped["action"] == 0).all() and swapped["n_done"] == 0
    c1 = Call(d.start_steps(list(range(0, K, 2)), stream=A, state=False))
    c2 = Call(d.process_steps(segs, CLC.NOW, stream=B, state=False))
    c3 = Call(d.timers_steps(CLC.NOW + 1000, stream=A))
    ready(A, B)
    ev = delayed(A)
    c1.issue()
    c2.issue()
    c3.issue()
    assert not ev.query(), "the delay on A ended before the chain was queued: lengthen it"
    (_, e1), (_, e2), (_, e3) = finish(c1, c2, c3)
    assert e1["n_markers"] == K // 2
    assert {int(s) for s in e2["state_after"][e2["action"] != 0]} == {TCL.TIME_WAIT, TCL.CLOSED}
    assert e3["n_done"] > 0 and set(int(s) for s in d.model.rows["state"][0:K:2]) == {TCL.CLOSED}


def test_arp_chain(closing, pair):
    """arp_query_start on A, arp_process of the replies on B, arp_lookup on A, then dk_arp_table_read with no explicit
    synchronize, which must show the replies' entries. With B first the replies are cached before the queries start, so
    no query sends a request."""
    A, B = pair
    d = arp_device(closing, K)
    warm_table(d, 4 * K)
    fr = arp_replies(K)
    m = copy.deepcopy(d.model)
    m.process(AC.model_frames(fr), 10)
    swapped = m.start(list(range(K)), 20)
    assert swapped["n_frames"] == 0 and swapped["n_ready"] == K
    ips = [ipv4(AC.host(1 + r)) for r in range(K)] + [ipv4(AC.host(999))]
    c1 = Call(d.start_steps(list(range(K)), 5, stream=A, state=False))
    c2 = Call(d.process_steps(fr, 10, stream=B, state=False))
    ready(A, B)
    ev = delayed(A)
    c1.issue()
    c2.issue()
    assert not ev.query(), "the delay on A ended before the chain was queued: lengthen it"
    found, macs = ARP.arp_lookup(d.table, ips, d.d_links, None, stream=A, fill=GA.FILL)
    table = d.table.as_map()
    (_, e1), (_, e2) = finish(c1, c2)
    assert e1["n_frames"] == K and e1["n_ready"] == 0 and e2["n_ready"] == K and e2["n_frames"] == K // 4
    assert table == d.model.table() and len(table) == K
    efound, emacs = d.model.lookup(ips, None)
    assert np.array_equal(found, efound) and np.array_equal(macs, emacs) and list(found) == [1] * K + [0]
    d.compare_state()


def test_arp_table_read_waits_for_the_other_stream(closing, pair):
    """dk_arp_table_read right behind an arp_process that is queued behind the delay: synchronous by contract."""
    A, B = pair
    d = arp_device(closing, K)
    c = Call(d.process_steps(arp_replies(K), 10, stream=A, state=False))
    ready(A)
    ev = delayed(A)
    c.issue()
    assert not ev.query(), "the delay on A ended before the call was queued: lengthen it"
    table = d.table.as_map()
    c.finish()
    assert table == d.model.table() and len(table) == K
    d.compare_state()


# ---- independent tables, shared pools ---------------------------------------------------------------------------------------
def test_independent_listen_tables(closing, pair):
    """Two tables, one driven on A behind the delay and one on B: B's calls complete while A's are pending."""
    A, B = pair
    (d1, f1), (d2, f2) = listen_device(closing), listen_device(closing)
    s1, a1, _ = listen_chain(d1, f1, K)
    s2, a2, _ = listen_chain(d2, f2, K, first=100)
    on_a = [Call(d1.process_steps(s1, T0, stream=A, state=False)), Call(d1.process_steps(a1, T0 + 10, stream=A))]
    on_b = [Call(d2.process_steps(s2, T0, stream=B, state=False)), Call(d2.process_steps(a2, T0 + 10, stream=B))]
    ready(A, B)
    ev = delayed(A)
    for ca, cb in zip(on_a, on_b):
        ca.issue()
        cb.issue()
    B.synchronize()
    assert not ev.query(), "the table on B waited for the table on A"
    finish(*on_a)
    finish(*on_b)


def test_independent_arp_tables(closing, pair):
    A, B = pair
    d1, d2 = arp_device(closing, K), arp_device(closing, K, first=500)
    warm_table(d1, 4 * K)
    warm_table(d2, 4 * K)
    on_a = [Call(d1.start_steps(list(range(K)), 5, stream=A, state=False)), Call(d1.process_steps(arp_replies(K), 10, stream=A))]
    on_b = [Call(d2.start_steps(list(range(K)), 5, stream=B, state=False)),
            Call(d2.process_steps(arp_replies(K, first=500), 10, stream=B))]
    ready(A, B)
    ev = delayed(A)
    for ca, cb in zip(on_a, on_b):
        ca.issue()
        cb.issue()
    B.synchronize()
    assert not ev.query(), "the table on B waited for the table on A"
    finish(*on_a)
    finish(*on_b)


def test_shared_connect_pool(closing, pair):
    """Two clients share the device's pool and alternate calls on A and B: each matches its own model."""
    A, B = pair
    warm_pools(closing)
    (d1, f1), (d2, f2) = connect_device(closing, K), connect_device(closing, K + 9, first=1000)
    calls = []
    for d, k, first, s in ((d1, K, 0, A), (d2, K + 9, 1000, B)):
        calls.append([Call(d.start_steps(list(range(k)), T0, stream=s, state=False)),
                      Call(d.process_steps(connect_answers(d, k, first), T0 + 100, stream=s, state=False)),
                      Call(d.timers_steps(T0 + 1000, stream=s, max_frames=k, max_ready=k))])
    ready(A, B)
    ev = delayed(A)
    for ca, cb in zip(*calls):
        ca.issue()
        cb.issue()
    assert not ev.query(), "the delay on A ended before the calls were queued: lengthen it"
    for cs in calls:
        out = finish(*cs)
        assert out[2][1]["n_frames"] > 0 and out[1][1]["n_ready"] > 0


def test_shared_close_pool(closing, pair):
    A, B = pair
    warm_pools(closing)
    (d1, t1), (d2, t2) = close_device(K, seed=41), close_device(K + 9, seed=42)
    calls = []
    for d, t, k, s in ((d1, t1, K, A), (d2, t2, K + 9, B)):
        calls.append([Call(d.start_steps(list(range(0, k, 2)), stream=s, state=False)),
                      Call(d.process_steps(close_answers(t, range(0, k, 2)), CLC.NOW, stream=s, state=False)),
                      Call(d.timers_steps(CLC.NOW + 1000, stream=s))])
    ready(A, B)
    ev = delayed(A)
    for ca, cb in zip(*calls):
        ca.issue()
        cb.issue()
    assert not ev.query(), "the delay on A ended before the calls were queued: lengthen it"
    for cs in calls:
        out = finish(*cs)
        assert out[2][1]["n_done"] > 0


# ---- growth of the scratch with work in flight ----------------------------------------------------------------------------
def streams_for(mode, pair):
    """(the three calls' streams, whether A is delayed first)."""
    A, B = pair
    return ((A, B, A), True) if mode == "in_flight" else ((A, A, A), False)


def growth(calls, streams, delay):
    """A small call, a call that needs far more scratch, a small call, issued with no host wait of the test's own; the
    delay (if any) is still pending when the growing call is made."""
    ready(*streams)
    ev = delayed(streams[0]) if delay else None
    calls[0].issue()
    assert ev is None or not ev.query(), "the delay on A ended before the growing call was made: lengthen it"
    calls[1].issue()
    calls[2].issue()
    return finish(*calls)


@pytest.mark.parametrize("mode", ["in_flight", "one_stream"])
def test_listen_scratch_growth(closing, pair, mode):
    (s0, s1, s2), delay = streams_for(mode, pair)
    d, flows = listen_device(closing, cap=4096, backlog=1000)
    syns, acks, _ = listen_chain(d, flows, 8)
    large = [LC.seg(LC.remote(100 + j // 2), 80 + (j // 2 & 1), LR.SYN if j % 7 else LR.ACK, seq=j) for j in range(LARGE)]
    calls = [Call(d.process_steps(syns, T0, stream=s0, state=False)), Call(d.process_steps(large, T0 + 5, stream=s1, state=False)),
             Call(d.process_steps(acks, T0 + 10, stream=s2))]
    (_, e0), (_, e1), (_, e2) = growth(calls, (s0, s1, s2), delay)
    assert e1["n_frames"] > LARGE // 4 and e1["n_ready"] > 8 and e2["n_ready"] == 8


@pytest.mark.parametrize("mode", ["in_flight", "one_stream"])
def test_connect_scratch_growth(closing, pair, mode):
    (s0, s1, s2), delay = streams_for(mode, pair)
    d, flows = connect_device(closing, 8)
    big, bflows = connect_device(closing, LARGE, first=100)
    calls = [Call(d.start_steps(list(range(8)), T0, stream=s0, state=False)),
             Call(big.start_steps(list(range(LARGE)), T0, stream=s1)),
             Call(d.process_steps(connect_answers(d, 8), T0 + 100, stream=s2))]
    (_, e0), (_, e1), (_, e2) = growth(calls, (s0, s1, s2), delay)
    assert e0["n_frames"] == 8 and e1["n_frames"] == LARGE and e2["n_ready"] > 0


@pytest.mark.parametrize("mode", ["in_flight", "one_stream"])
def test_close_scratch_growth(closing, pair, mode):
    (s0, s1, s2), delay = streams_for(mode, pair)
    d, t = close_device(8, seed=51)
    big, tb = close_device(LARGE, seed=52)
    calls = [Call(d.start_steps(list(range(8)), stream=s0, state=False)),
             Call(big.start_steps(list(range(LARGE)), stream=s1)),
             Call(d.process_steps(close_answers(t, range(8)), CLC.NOW, stream=s2))]
    (_, e0), (_, e1), (_, e2) = growth(calls, (s0, s1, s2), delay)
    assert e0["n_markers"] == 8 and e1["n_markers"] == LARGE and e2["n_done"] > 0


@pytest.mark.parametrize("mode", ["in_flight", "one_stream"])
def test_arp_scratch_growth(closing, pair, mode):
    (s0, s1, s2), delay = streams_for(mode, pair)
    d = arp_device(closing, 8, cap=4096, extra_rows=LARGE)
    large = list(range(8, 8 + LARGE))
    calls = [Call(d.start_steps(list(range(8)), 5, stream=s0, state=False)),
             Call(d.start_steps(large, 6, stream=s1, state=False)),
             Call(d.process_steps(arp_replies(8), 10, stream=s2))]
    (_, e0), (_, e1), (_, e2) = growth(calls, (s0, s1, s2), delay)
    assert e0["n_frames"] == 8 and e1["n_frames"] == LARGE and e2["n_ready"] == 8


# ---- C. the wrappers' own outputs on a side stream ------------------------------------------------------------------------
def test_close_start_outputs_on_a_side_stream(pair):
    """close_start makes its status words, marker list and n_markers itself. With the current stream busy and the call
    on a side stream, fills queued on the current stream would land after the kernel's stores and erase them."""
    import torch

    cur, side = pair
    d, t = close_device(3 * K)
    close = list(range(0, 3 * K, 2)) + [3 * K + 5]
    torch.cuda.synchronize()
    with torch.cuda.stream(cur):
        c = Call(d.start_steps(close, stream=side))
        ready(side)
        ev = delayed(cur)
        c.issue()
        pending = not ev.query()
        s, exp = c.finish()  # compares the statuses, the markers, n_markers and the canary beyond them
    assert pending, "the delay on the current stream ended before the call was queued: lengthen it"
    assert exp["n_markers"] == 3 * K // 2 and exp["status"][-1] == TCL.E_ROW


def test_listen_release_outputs_on_a_side_stream(closing, pair):
    import torch

    cur, side = pair
    d, flows = listen_device(closing)
    syns, acks, keys = listen_chain(d, flows, K)
    d.process(syns, T0)
    torch.cuda.synchronize()
    with torch.cuda.stream(cur):
        ready(side)
        ev = delayed(cur)
        pending = not ev.query()
        found = d.release(keys, stream=side)
    assert pending, "the delay on the current stream ended before the call was made: lengthen it"
    assert [int(x) for x in found] == [1] * (len(keys) - 1) + [0]


def test_arp_lookup_outputs_on_a_side_stream(closing, pair):
    import torch

    cur, side = pair
    d = arp_device(closing, K)
    d.process(arp_replies(K), 10)
    torch.cuda.synchronize()
    ips = [AC.host(1 + r) for r in range(K)] + [AC.host(999)]
    with torch.cuda.stream(cur):
        ready(side)
        ev = delayed(cur)
        pending = not ev.query()
        found, macs = d.lookup(ips, [r if r < 6 and r % 2 else AR.NO_LINK for r in range(K + 1)], stream=side)
    assert pending, "the delay on the current stream ended before the call was made: lengthen it"
    assert list(found) == [1] * K + [0]
