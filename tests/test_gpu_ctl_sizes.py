"""The 13 asynchronous entry points of the four control-plane families (listen, connect, close, ARP) on both sides of the
scan tile. Every call compacts its outputs with dk_tcp_tx_scan, whose tile is 1,024 items: past one tile the scan takes
its block-sum spine and tile-offset path and grid_for gives several workgroups. Each call is run at 1,023, 1,024, 1,025
and 2,049 scanned items (one short of a tile, one tile, two tiles with a single item in the second, three tiles) through
the families' own harnesses, so every comparison is theirs: bit-exact against the CPU model over canary fills, the whole
output blob, and the tables afterwards. Outcomes vary with the item's index, and each test asserts on the model's answer
that the compacted outputs come from items on both sides of index 1,024.

Largest item count each entry point is run at, before this module and with it ("item" is what the call's scan runs
over; the two lookups have no scan, their item is a key):

    call                    item           before    with
    dk_tcp_listen_process   frames          2,057    2,057  (test_gpu_tcp_listen, unchanged)
    dk_tcp_listen_timers    table slots       512    4,096  (slots are a power of two: 1,024, 2,048 and 4,096 are run)
    dk_tcp_listen_release   keys                4    2,049
    dk_tcp_connect_start    start entries     140    2,049
    dk_tcp_connect_process  frames      about 565    2,049
    dk_tcp_connect_timers   table rows        150    2,049
    dk_tcp_close_start      close entries     700    2,049
    dk_tcp_close_process    frames         23,640   23,640  (test_gpu_tcp_close, unchanged)
    dk_tcp_close_timers     table rows      1,100    2,049
    dk_arp_process          frames            300    2,049
    dk_arp_query_start      start entries       8    2,049
    dk_arp_timers           query rows         75    2,049
    dk_arp_lookup           keys               60    2,049

A listen table's slot count is a power of two, so dk_tcp_listen_timers cannot be run at the four sizes: it is run at one
tile, two tiles and at 4,096 slots, the smallest table of at least 2,049. Its frames and records are reported by slot,
which the model does not know, so there the two sides of slot 1,024 are asserted on the device's answer.

Each family's one-short capacity case is repeated once at 1,025 items for max_frames: the call reports its need and
writes nothing else."""
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
from demikernel_amd import arp as ARP
from demikernel_amd import tcp_close as TCL
from demikernel_amd import tcp_connect as TC
from demikernel_amd import tcp_listen as TL

pytestmark = pytest.mark.gpu

TILE = 1024
SIZES = [1023, 1024, 1025, 2049]
BIG = 1 << 20


def both_sides(n, **outputs):
    """Each of the call's compacted outputs (name=indices of the items that gave one) comes from some of the n items
    and not from all, so the scanned flags are neither all 0 nor all 1, and from the first tile. At 2,049 items each
    also comes from the second tile. At 1,025 and 2,049 the last tile holds a single item, which gives one output or
    another: that item has one."""
    last = -1
    for what, idx in outputs.items():
        idx = np.asarray(sorted(int(i) for i in idx))
        assert 0 < len(idx) < n, (what, len(idx), n)
        assert idx.min() < TILE and idx.max() < n, (what, idx.min(), idx.max())
        if n > 2 * TILE:
            assert ((idx >= TILE) & (idx < 2 * TILE)).any(), what
        last = max(last, int(idx.max()))
    assert last == n - 1 or n <= TILE, (last, sorted(outputs))


@pytest.fixture
def closing():
    made = []
    yield made.append
    for d in made:
        d.close()


# ---- listen ---------------------------------------------------------------------------------------------------------------
def listen_device(closing, cap, backlog, **fields):
    flows, L, lsn = LC.server([80, 81], max_backlog=backlog, isn_counter=[0xFF00, 3], nonce=[0x1234, 0xCAFEF00D], **fields)
    d = GL.Device(flows, L, lsn, cap=cap)
    closing(d)
    return d, L


@pytest.mark.parametrize("cap", [1024, 2048, 4096])
def test_listen_timers(closing, cap):
    """3 * cap / 8 half-open entries of two listeners, the earlier half due: listener 0's resend, listener 1's (no
    retries) time out, so both scans over the slots have flags set among flags clear."""
    T0 = 1_000_000
    d, L = listen_device(closing, cap, [cap // 4, cap // 8], handshake_retries=[1, 0], handshake_timeout_ns=[1000, 1000])
    m = cap // 4
    early = [LC.seg(LC.remote(k), 80 + (k % 3 == 2), LR.SYN, seq=k) for k in range(0, m, 2)]
    late = [LC.seg(LC.remote(k), 80 + (k % 3 == 2), LR.SYN, seq=k) for k in range(1, m, 2)]
    d.process(early, T0)
    d.process(late, T0 + 5)
    got, exp, _ = d.timers(T0 + 1000, max_frames=m, max_ready=m)  # the early entries' deadline equals now
    assert exp["fits"] and exp["n_frames"] + exp["n_ready"] == len(early) and min(exp["n_frames"], exp["n_ready"]) > m // 8
    for what, slots in (("frames", got["frame_seg"][:exp["n_frames"]]), ("records", got["ready"]["slot"][:exp["n_ready"]])):
        assert slots.max() < cap
        if cap > TILE:  # the sweep's items are slots: both sides of slot 1,024 gave outputs
            assert slots.min() < TILE <= slots.max(), what
    got, exp, _ = d.timers(T0 + 1005, max_frames=m, max_ready=m)  # the late entries
    assert exp["n_frames"] + exp["n_ready"] == len(late)
    got, exp, _ = d.timers(T0 + 2005, max_frames=m - 1, max_ready=m)  # every resent entry times out: records alone
    assert exp["fits"] and exp["n_frames"] == 0 and exp["n_ready"] > m // 2


@pytest.mark.parametrize("n", SIZES)
def test_listen_release(closing, n):
    """n keys, every other one in the table: one thread per key over several workgroups, found[] against the model,
    the released slots tombstones and the listeners' inflight counts afterwards."""
    m = (n + 1) // 2
    d, L = listen_device(closing, 4096, [1024, 512])
    d.process([LC.seg(LC.remote(k), 80 + (k % 3 == 2), LR.SYN, seq=k) for k in range(m)])
    have = [TL.key(int(k % 3 == 2), *LC.remote(k)) for k in range(m)]
    assert set(have) == set(d.model.conns)
    keys = [have[(i // 2 * 7919) % m] if i % 2 == 0 else TL.key(i % 2 + i % 3 // 2, *LC.remote(5000 + i)) for i in range(n)]
    assert len(set(keys)) == n
    found = d.release(keys)
    both_sides(n, found=np.nonzero(found)[0])
    assert len(d.model.conns) == 0 and int(d.model.listeners["inflight"].sum()) == 0


def test_listen_one_short_at_1025(closing):
    n = 1025
    d, L = listen_device(closing, 2048, [600, 300])
    fr = []
    for i in range(n):
        k = i // 2 if i % 5 else i // 3  # repeats: later SYNs of a key are handshake segments
        fr.append(LC.seg(LC.remote(k), 80 + (k & 1), LR.SYN if i % 7 else LR.ACK, seq=i))
    rx, _ = d.receive(fr)
    need = copy.deepcopy(d.model).process(rx.to_numpy(), d.lsn, LC.NOW, LC.LINKS, slot_stride=64, max_frames=BIG,
                                          out_bytes=1 << 30, max_ready=BIG)
    nf, nr = need["n_frames"], need["n_ready"]
    both_sides(n, frames=need["frame_seg"], records=np.nonzero(np.isin(need["action"], (TL.ESTABLISHED, TL.BAD_ACK)))[0])
    assert nr > 8
    rows_before = d.table.rows().tobytes()
    got, exp = d.process(fr, max_frames=nf - 1, max_ready=nr, out_size=nf * 64 + 64)  # the harness: nothing else written
    assert not exp["fits"] and (got["n_frames"], got["n_ready"]) == (nf, nr) and set(got["status"]) == {TL.NO_ROOM}
    assert d.table.rows().tobytes() == rows_before
    got, exp = d.process(fr, max_frames=nf, max_ready=nr, out_size=nf * 64 + 64)
    assert exp["fits"] and set(got["status"]) == {TL.OK}


# ---- connect --------------------------------------------------------------------------------------------------------------
T0 = 1_000_000


def connect_device(closing, n):
    """n rows: a few CLOSED (E_STATE), every 11th with no retries (a record at start), timeouts of 1,000 and 2,000 ns
    by row parity; the ISN counter wraps half way through a start of all rows."""
    i = np.arange(n)
    flows, rows, cmap = CC.client(n, handshake_retries=np.where(i % 11 == 3, 0, 1 + i % 3), link=i % 2,
                                  window_scale=i % 15, handshake_timeout_ns=1000 + (i % 2) * 1000)
    rows["state"][i % 13 == 5] = TC.CLOSED
    d = GC.Device(flows, rows, cmap, nonce=0xC0FFEE11, counter=(0x10000 - n // 2) & 0xFFFF)
    closing(d)
    start = list(range(n))
    start[7], start[9] = n + 3, 8  # beyond the table; a row named twice
    return d, start


def connect_frames(d, n):
    """n frames, in row order: per CONNECTING row a SYN+ACK, a RST, a stray ACK, another SYN+ACK or nothing, by the
    row's distance from the last but one; traffic of no row spread between them. The last frame is the last but one
    row's SYN+ACK; the last row gets no frame, so its timer runs."""
    rows = d.model.rows
    own = []
    for r in range(n):
        if int(rows[r]["state"]) != TC.CONNECTING:
            continue
        a, kind = int(rows[r]["local_isn"]) + 1, (n - 2 - r) % 5
        if kind in (0, 3):
            own.append(CC.seg(r, CR.SYN | CR.ACK, seq=r * 977, ack=a, options=CC.OPT_MSS_WS0 if kind else b""))
        elif kind == 1:
            own.append(CC.seg(r, CR.RST | CR.ACK, seq=5, ack=a))
        elif kind == 2:
            own.append(CC.seg(r, CR.ACK, seq=5, ack=a + 7))
    no = n - len(own)
    assert 0 < no < n // 2
    fr, own = [], own[::-1]
    for j in range(n - 1, -1, -1):  # other traffic evenly spread, counted from the end: the last frame is a row's
        fr.append(CC.OTHER[j % len(CC.OTHER)] if (j + 1) * no // n != j * no // n else own.pop())
    assert not own and len(fr) == n
    return fr


@pytest.mark.parametrize("n", SIZES)
def test_connect_start_process_timers(closing, n):
    """connect_start of n entries with the ISN counter wrapping inside the batch, connect_process of n frames (one
    SYN+ACK, RST or stray ACK per row plus foreign traffic), connect_timers over the n rows with deadlines on both
    sides of now."""
    d, start = connect_device(closing, n)
    c0 = d.model.counter
    got, exp = d.start(start, T0)
    assert exp["fits"] and {int(s) for s in exp["status"]} == {TC.OK, TC.E_ROW, TC.E_STATE}
    assert d.model.counter == (c0 + n) & 0xFFFF < c0  # the counter wrapped
    both_sides(n, syns=exp["frame_seg"], records=[int(y["frame"]) for y in exp["ready"]])
    fr = connect_frames(d, n)
    got, exp = d.process(fr, T0 + 100)
    assert exp["fits"] and {int(a) for a in exp["action"]} >= {TC.SKIP, TC.ESTABLISHED, TC.REFUSED, TC.RETRY_SYN, TC.EXHAUSTED}
    both_sides(n, frames=exp["frame_seg"], records=[int(y["frame"]) for y in exp["ready"]])
    assert exp["action"][n - 1] == TC.ESTABLISHED  # the single item of the second tile gives a frame and a record
    # even rows left alone are due (T0 + 1,000), odd ones not (T0 + 2,000); retried rows: T0 + 1,100 and T0 + 2,100
    got, exp = d.timers(T0 + 1500, max_frames=n, max_ready=n)
    assert exp["fits"]
    both_sides(n, syns=exp["frame_seg"], records=[int(y["row"]) for y in exp["ready"]])
    assert (d.model.rows["state"] == TC.CONNECTING).sum() > n // 8  # and rows on the other side of now remain


def test_connect_one_short_at_1025(closing):
    n = 1025
    d, start = connect_device(closing, n)
    need = copy.deepcopy(d.model).start(start, T0, CC.LINKS, slot_stride=64, max_frames=BIG, out_bytes=1 << 40, max_ready=BIG)
    nf, nr = need["n_frames"], need["n_ready"]
    assert nf > TILE // 2 and nr > 8 and need["frame_seg"][-1] >= TILE
    before = TC.rows_to_host(d.d_rows).tobytes()
    got, exp = d.start(start, T0, max_frames=nf - 1, max_ready=nr, out_size=nf * 64 + 64)
    assert not exp["fits"] and (got["n_frames"], got["n_ready"]) == (nf, nr)
    assert set(got["status"]) == {TC.NO_ROOM, TC.E_ROW, TC.E_STATE} and TC.rows_to_host(d.d_rows).tobytes() == before
    got, exp = d.start(start, T0, max_frames=nf, max_ready=nr, out_size=nf * 64 + 64)
    assert exp["fits"]


# ---- close ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_close_start(n):
    """n close entries over 2 n connections: E_ORDER (a duplicate and a descent), E_STATE and E_BADF among the accepted
    ones, the marker list compacted from both sides of the tile boundary. An entry beyond the table (E_ROW) puts every
    later one out of order, so it can only be the last: it is, where the last tile holds more than that one item."""
    d = GCL.Device(GCL.start_table(2 * n))
    close = list(range(0, 2 * n, 2))
    close[3] = close[2]
    close[n // 2] = 1
    if n <= TILE:
        close[n - 1] = 2 * n + 5
    s, exp = d.start(close)
    assert {TCL.OK, TCL.E_ORDER, TCL.E_STATE, TCL.E_BADF} <= {int(x) for x in exp["status"]}
    assert (exp["status"][n - 1] == TCL.E_ROW) == (n <= TILE)
    ok = np.nonzero(exp["status"] == TCL.OK)[0]
    both_sides(n, markers=ok)
    assert ok.max() >= n - 3
    assert exp["n_markers"] == int((exp["status"] == TCL.OK).sum())


@pytest.mark.parametrize("n", SIZES)
def test_close_timers(n):
    """n rows, TIME-WAIT deadlines at now - 1, now and now + 1, CLOSED rows retired once. The states' phase puts a
    due row last."""
    now = 1 << 41
    c = np.arange(n) + (1 - n) % 7
    S = (TCL.TIME_WAIT, TCL.TIME_WAIT, TCL.TIME_WAIT, TCL.CLOSED, TCL.FIN_WAIT_1, TCL.IDLE, TCL.FAULT)
    t = CLC.table([S[k % 7] for k in c], seed=n)
    t["rows"]["deadline_ns"] = np.where(c % 7 == 0, now, np.where(c % 7 == 1, now - 1, now + 1))
    t["rows"]["flags"] = np.where(c % 21 == 3, TCL.RETIRED, 0)
    d = GCL.Device(t)
    need = copy.deepcopy(d.model).timers(now, max_done=BIG)["n_done"]
    got, exp = d.timers(now, max_done=need - 1)
    assert not exp["fits"] and exp["n_done"] == need
    got, exp = d.timers(now, max_done=need)
    assert exp["fits"] and exp["n_done"] == need
    both_sides(n, done=[int(y["row"]) for y in exp["done"]])
    got, exp = d.timers(now + 1)
    assert exp["n_done"] == int((c % 7 == 2).sum())


def test_close_one_short_at_1025():
    n = 1025
    states = [(TCL.FIN_WAIT_1, TCL.FIN_WAIT_2, TCL.CLOSING, TCL.LAST_ACK, TCL.IDLE, TCL.TIME_WAIT)[c % 6] for c in range(260)]
    t = CLC.table(states + [TCL.FIN_WAIT_2], seed=1025)
    scripts = [[CLC.seg(t, c, CLC.KINDS[(c // 6 + j) % 6], j) for j in range(4)] for c in range(260)]
    segs = CLC.interleave(scripts, pad_every=9)[:n - 1] + [CLC.seg(t, 260, "F")]  # the last frame: a FIN, acknowledged
    assert len(segs) == n
    d = GCL.Device(t)
    need = copy.deepcopy(d.model).process(CLC.rx_arrays(segs, t["nconns"]), CLC.NOW, CLC.LINKS, slot_stride=64,
                                          max_frames=BIG, out_bytes=1 << 30, max_done=BIG,
                                          action_in=(np.arange(n) * 7 % 13).astype(np.uint8))
    nf, nd = need["n_frames"], need["n_done"]
    both_sides(n, acks=need["frame_seg"], done=[int(y["frame"]) for y in need["done"]])
    assert nd > 8
    got, exp = d.process(segs, max_frames=nf - 1, max_done=nd, out_size=nf * 64 + 64)  # the harness: nothing else written
    assert not exp["fits"] and (got["n_frames"], got["n_done"]) == (nf, nd) and TCL.NO_ROOM in set(got["status"])
    got, exp = d.process(segs, max_frames=nf, max_done=nd, out_size=nf * 64 + 64)
    assert exp["fits"]


# ---- ARP ------------------------------------------------------------------------------------------------------------------
NLINKS = 64  # a link belongs to one address: two rows that resolve to different MACs never share one


def row_links(n):
    return [r if r < NLINKS and r % 5 != 4 else AR.NO_LINK for r in range(n)]


def arp_device(closing, case):
    d = GA.Device(case)
    closing(d)
    return d


def arp_process_case(n):
    """n frames of n // 3 senders, so that every sender's frames lie a third of the batch apart and its last writer
    is in another tile than its first; each frame carries its own sha. A third are addressed to us, every tenth is
    no ARP frame; 50 senders have an entry that expires at the batch's clock. n // 2 + 1 WAITING rows, several per
    address."""
    S = n // 3
    fr = []
    for i in range(n):
        s = AC.host(1 + i % S)
        if i % 10 == 9:
            fr.append(AC.F.tcp_frame(b"abc"))
        else:
            fr.append((AC.req if i % 2 else AC.rep)(s, AC.ALICE if i % 3 == 0 else AC.host(70000 + i), sha=AC.mac_of(i)))
    fr[n - 1] = AC.req(AC.host(1 + (n - 1) % S), AC.ALICE, sha=AC.mac_of(n - 1))  # the last frame is answered
    nr = n // 2 + 1
    who = [(r * 5) % (S + 40) for r in range(nr)]  # a link per address: rows of one address wake with one MAC
    rows = AC.waiting([AC.host(1 + w) for w in who], links=[w if w < NLINKS and w % 5 != 4 else AR.NO_LINK for w in who])
    initial = [(AC.host(1 + k), AC.mac_of(900000 + k)) for k in range(0, 100, 2)]
    return S, fr, AC.Case(f"process_{n}", cap=2048, initial=initial, rows=rows, links=AC.links_of(NLINKS))


@pytest.mark.parametrize("n", SIZES)
def test_arp_process(closing, n):
    S, fr, case = arp_process_case(n)
    assert ARP.fits(case.cap, S + len(case.initial))
    d = arp_device(closing, case)
    got, exp = d.process(fr, AC.TTL)
    assert exp["fits"] and {int(a) for a in exp["action"]} >= {ARP.SKIP, ARP.DROPPED, ARP.HIT | ARP.INSERTED,
                                                              ARP.LEARNED | ARP.INSERTED, ARP.LEARNED | ARP.INSERTED | ARP.REPLY}
    woke = [int(y["frame"]) for y in exp["ready"]]
    both_sides(n, replies=exp["frame_seg"])
    assert len(woke) > len(case.rows) // 2 and min(woke) < 8 and len(set(woke)) > 64
    if n > 2 * TILE:
        assert len(case.rows) > TILE and len(woke) > TILE // 2  # the sort of the query rows and arp_wake pass one tile
    table = d.model.table()
    last = {}
    for i, f in enumerate(AC.model_frames(fr)):
        if f.covered and exp["action"][i] & ARP.INSERTED:
            last[f.spa] = i
    assert all(table[ip][0] == AC.mac_of(i) for ip, i in last.items())
    if n > TILE:  # senders first written in the first tile and last written in another
        assert sum(1 for i in last.values() if i >= TILE) > (8 if n > 2 * TILE else 0)
    d.lookup([AC.host(1 + k) for k in range(S + 40)])


@pytest.mark.parametrize("n", SIZES)
def test_arp_query_start(closing, n):
    """n start entries: rows whose address is cached resolve at once (records), the others send a request (frames);
    E_ROW, E_STATE (a row named twice, rows already WAITING) and E_LINK among them."""
    rows = AC.idle([AC.host(1 + r) for r in range(n)], links=row_links(n))
    rows["state"][np.arange(n) % 17 == 6] = AR.WAITING
    rows["link"][np.arange(n) % 19 == 7] = 1000
    initial = [(AC.host(1 + k), AC.mac_of(k)) for k in range(0, n, 3)]
    d = arp_device(closing, AC.Case(f"start_{n}", cap=2048, initial=initial, rows=rows, links=AC.links_of(NLINKS)))
    start = list(range(n))
    start[5], start[n - 4] = n + 1, n - 6
    got, exp = d.start(start, 77)
    assert exp["fits"] and {int(s) for s in exp["status"]} == {AR.OK, AR.E_ROW, AR.E_STATE, AR.E_LINK}
    both_sides(n, requests=exp["frame_seg"], resolved=[start.index(int(y["row"])) for y in exp["ready"]])


@pytest.mark.parametrize("n", SIZES)
def test_arp_timers(closing, n):
    """n rows with deadlines at now - 1, now and now + 1 and 1 to 3 requests sent: re-sends, re-sends that find the
    address cached meanwhile, and ETIMEDOUT records."""
    r = np.arange(n)
    rows = AC.waiting([AC.host(1 + k) for k in range(n)], links=row_links(n))
    rows["deadline_ns"] = AC.SEC + (r + 2) % 3 - 1
    rows["sent"] = 1 + (r // 3) % 3
    rows["state"][r % 23 == 11] = AR.IDLE
    initial = [(AC.host(1 + k), AC.mac_of(k)) for k in range(0, n, 5)]
    d = arp_device(closing, AC.Case(f"timers_{n}", cap=2048, retries=2, initial=initial, rows=rows, links=AC.links_of(NLINKS)))
    got, exp = d.timers(AC.SEC, max_frames=n, max_ready=n)
    assert exp["fits"]
    both_sides(n, requests=exp["frame_seg"], records=[int(y["row"]) for y in exp["ready"]])
    assert {int(y["err"]) for y in exp["ready"]} == {0, 110}
    assert (d.model.rows["state"] == AR.WAITING).sum() > n // 4


@pytest.mark.parametrize("n", SIZES)
def test_arp_lookup(closing, n):
    """n addresses, every other one cached, each found one writing a link of its own."""
    initial = [(AC.host(1 + k), AC.mac_of(k)) for k in range(0, n, 2)]
    d = arp_device(closing, AC.Case(f"lookup_{n}", cap=4096, initial=initial, links=AC.links_of(n)))
    link = [k if k % 3 else AR.NO_LINK for k in range(n)]
    found, macs = d.lookup([AC.host(1 + k) for k in range(n)], link)
    both_sides(n, found=np.nonzero(found)[0])


def test_arp_one_short_at_1025(closing):
    n = 1025
    S, fr, case = arp_process_case(n)
    d = arp_device(closing, case)
    need = copy.deepcopy(d.model).process(AC.model_frames(fr), AC.TTL, max_frames=BIG, max_ready=BIG)
    nf, nr = need["n_frames"], need["n_ready"]
    both_sides(n, replies=need["frame_seg"])
    assert nr > 8
    got, exp = d.process(fr, AC.TTL, max_frames=nf - 1, max_ready=nr)  # the harness: nothing else is written
    assert not exp["fits"] and got["status"][0] == AR.NO_ROOM
    assert (got["n_frames"], got["n_ready"], got["n_entries"]) == (nf, nr, need["n_entries"])
    got, exp = d.process(fr, AC.TTL, max_frames=nf, max_ready=nr)
    assert exp["fits"] and got["status"][0] == AR.OK
