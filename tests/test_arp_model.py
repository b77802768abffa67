"""tests/arp_reference.py pinned against the reference's own scripted expectations (arp/tests.rs and the tests of
collections/hashttlcache.rs), re-expressed by hand as data, plus the cases include/dk_arp.h spells out. The expected
bytes and tables below are written down here, never computed by the model."""
import errno

import arp_cases as C
import arp_reference as R
from demikernel_amd.rx import ipv4

A, B, CA = C.ALICE, C.BOB, C.CARRIE
AM, BM, CM = C.ALICE_MAC, C.BOB_MAC, C.CARRIE_MAC
IP = lambda a: bytes(int(x) for x in a.split("."))  # noqa: E731
ARP_HEAD = bytes([0x08, 0x06, 0x00, 0x01, 0x08, 0x00, 0x06, 0x04])
FF = b"\xff" * 6


def reply_bytes(local, local_mac, remote, remote_mac):
    return remote_mac + local_mac + ARP_HEAD + b"\x00\x02" + local_mac + IP(local) + remote_mac + IP(remote)


def request_bytes(local, local_mac, target):
    return FF + local_mac + ARP_HEAD + b"\x00\x01" + local_mac + IP(local) + FF + IP(target)


def only(case):
    m, outs = C.run_model(case)
    return m, outs[-1]


# ---- arp/tests.rs ----------------------------------------------------------------------------------------------------
def test_arp_immediate_reply():
    m, o = only(C.immediate_reply())
    assert o["frames"] == [reply_bytes(A, AM, B, BM)] and len(o["frames"][0]) == 42
    assert list(o["action"]) == [R.LEARNED | R.INSERTED | R.REPLY] and list(o["reply_frame"]) == [0]
    assert (o["n_frames"], o["n_ready"], o["n_entries"], o["fits"]) == (1, 0, 1, True)


def test_arp_no_reply():
    m, o = only(C.no_reply())
    assert o["frames"] == [] and list(o["action"]) == [R.DROPPED] and m.table() == {}
    assert list(o["reply_frame"]) == [R.NONE]


def test_arp_cache_update():
    m, o = only(C.cache_update())
    assert {k: v[0] for k, v in m.table().items()} == {ipv4(CA): CM}
    assert o["frames"] == [reply_bytes(B, BM, CA, CM)]


def test_arp_cache_timeout():
    """Retry count 2, 1 s timeout: three requests, then ETIMEDOUT with no fourth frame."""
    m, outs = C.run_model(C.query_timeout())
    want = request_bytes(A, AM, CA)
    assert [o["frames"] for o in outs] == [[want], [want], [want], [], []]
    assert [len(o["ready"]) for o in outs] == [0, 0, 0, 1, 0]
    y = outs[3]["ready"][0]
    assert (int(y["row"]), int(y["err"]), int(y["frame"]), int(y["ip"])) == (0, errno.ETIMEDOUT, R.NONE, ipv4(CA))
    assert (int(m.rows[0]["state"]), int(m.rows[0]["err"]), int(m.rows[0]["sent"])) == (R.FAILED, errno.ETIMEDOUT, 3)
    assert [int(o["status"][0]) for o in outs] == [R.OK] * 5


# ---- collections/hashttlcache.rs -------------------------------------------------------------------------------------
def test_ttl_cache_evicts_by_default_ttl_exactly_at_expiration():
    c = R.TtlCache(100, 10)
    c.insert("a", 1)
    c.advance_clock(109)
    c.cleanup()
    assert c.get("a") == 1
    c.advance_clock(110)
    c.cleanup()
    assert c.get("a") is None


def test_ttl_cache_evicts_by_explicit_ttl():
    c = R.TtlCache(100, 10)
    c.insert_with_ttl("a", 1, 3)
    c.advance_clock(102)
    c.cleanup()
    assert c.get("a") == 1
    c.advance_clock(103)
    c.cleanup()
    assert c.get("a") is None


def test_ttl_cache_without_ttl_never_evicts():
    c = R.TtlCache(100, None)
    c.insert("a", 1)
    c.insert_with_ttl("b", 2, None)
    c.advance_clock(1 << 62)
    c.cleanup()
    assert (c.get("a"), c.get("b")) == (1, 2)


def test_ttl_cache_replaced_entry_takes_the_new_expiration():
    c = R.TtlCache(100, 10)
    c.insert("a", 1)
    c.advance_clock(105)
    assert c.insert("a", 2) == 1
    c.advance_clock(112)
    c.cleanup()
    assert c.get("a") == 2
    c.advance_clock(115)
    c.cleanup()
    assert c.get("a") is None


# ---- what dk_arp.h spells out ------------------------------------------------------------------------------------------
def test_expired_entry_answers_get_until_the_next_insert():
    m, outs = C.run_model(C.expired_still_answers())
    assert list(outs[0]["action"]) == [R.DROPPED] and m.table() == {ipv4(B): (BM, C.TTL)}
    found, macs = outs[1]
    assert list(found) == [1, 0] and bytes(macs[0]) == BM and bytes(macs[1]) == bytes(6)
    s = outs[2]
    assert (s["n_frames"], s["n_ready"]) == (1, 1) and s["frames"] == [request_bytes(A, AM, CA)] and s["frame_seg"] == [1]
    assert int(m.rows[0]["state"]) == R.RESOLVED and bytes(m.rows[0]["mac"]) == BM
    assert bytes(m.links[0]["dst_mac"]) == BM                      # the start wrote the row's link
    assert bytes(m.links[1]["dst_mac"]) == BM                      # the lookup wrote link 1 for BOB; CARRIE was not found
    assert bytes(m.links[0]["src_mac"]) == bytes(range(0x18, 0x1E)) and int(m.links[0]["reserved"]) == 0xC0DE0000
    assert (int(m.rows[1]["state"]), int(m.rows[1]["sent"]), int(m.rows[1]["deadline_ns"])) == (R.WAITING, 1, 5 + C.SEC)


def test_first_insert_of_a_batch_removes_expired_entries_of_other_keys():
    m, outs = C.run_model(C.first_insert_cleans_others())
    assert list(outs[0]["action"]) == [R.DROPPED, R.LEARNED | R.INSERTED]
    assert m.table() == {ipv4(C.host(3)): (C.mac_of(ipv4(C.host(3))), 2 * C.TTL)} and outs[0]["n_entries"] == 1
    assert list(outs[1][0]) == [0, 0, 1]
    m, o = only(C.one_tick_early())
    assert set(m.table()) == {ipv4(B), ipv4(C.host(3))} and m.table()[ipv4(B)] == (BM, C.TTL)


def test_f0_sees_its_own_expired_entry():
    m, o = only(C.f0_expired_hit())
    assert list(o["action"]) == [R.HIT | R.INSERTED, R.DROPPED, R.HIT | R.INSERTED]
    assert m.table() == {ipv4(B): (C.mac_of(8), 2 * C.TTL + 5)}


def test_replies_from_unknown_senders():
    m, o = only(C.reply_to_us_unknown())
    assert list(o["action"]) == [R.LEARNED | R.INSERTED] and o["frames"] == [] and m.table() == {ipv4(B): (BM, 7 + C.TTL)}
    m, o = only(C.reply_other_unknown())
    assert list(o["action"]) == [R.DROPPED] and o["frames"] == [] and m.table() == {}


def test_row_keeps_the_first_waking_mac():
    m, o = only(C.first_waking_mac())
    assert bytes(m.rows[0]["mac"]) == C.mac_of(1) and bytes(m.links[1]["dst_mac"]) == C.mac_of(1)
    assert m.table()[ipv4(B)][0] == C.mac_of(2)
    assert len(o["ready"]) == 1 and (int(o["ready"][0]["frame"]), bytes(o["ready"][0]["mac"])) == (0, C.mac_of(1))
    assert list(o["action"]) == [R.LEARNED | R.INSERTED, R.HIT | R.INSERTED]
    assert bytes(m.links[0].tobytes()) == C.links_of(2)[0].tobytes()  # an untouched link


def test_disabled():
    m, outs = C.run_model(C.disabled())
    s, p, (found, macs) = outs
    assert (s["n_frames"], s["n_ready"]) == (0, 1) and bytes(s["ready"][0]["mac"]) == bytes(6)
    assert list(p["action"]) == [R.HIT | R.INSERTED | R.REPLY, R.HIT | R.INSERTED, R.HIT | R.INSERTED]
    assert p["frames"] == [reply_bytes(A, AM, B, BM)] and p["n_entries"] == 0 and m.table() == {}
    assert len(p["ready"]) == 1 and (int(p["ready"][0]["row"]), bytes(p["ready"][0]["mac"])) == (1, BM)
    assert list(found) == [1, 1] and not macs.any() and not m.links[0]["dst_mac"].any()


def test_timers_cache_look_after_the_resend_resolves():
    m, outs = C.run_model(C.timers_lookup_resolves())
    o = outs[1]
    assert o["frames"] == [request_bytes(A, AM, B), request_bytes(A, AM, CA)] and o["frame_seg"] == [0, 1]
    assert len(o["ready"]) == 1 and (int(o["ready"][0]["row"]), int(o["ready"][0]["err"])) == (0, 0)
    assert [int(s) for s in m.rows["state"]] == [R.RESOLVED, R.WAITING] and [int(s) for s in m.rows["sent"]] == [2, 2]
    assert bytes(m.links[0]["dst_mac"]) == BM and int(m.rows[1]["deadline_ns"]) == 2 * C.SEC


def test_capacity_is_all_or_nothing_in_the_model():
    case = C.first_waking_mac()
    case.steps = [("process", case.steps[0][1], 3, {"max_ready": 0})]
    m, o = only(case)
    assert not o["fits"] and int(o["status"][0]) == R.NO_ROOM and (o["n_ready"], o["n_entries"]) == (1, 1)
    assert m.table() == {} and m.rows.tobytes() == case.rows.tobytes() and m.links.tobytes() == case.links.tobytes()


def test_device_shapes_run_through_the_model():
    for make in C.DEVICE_CASES:
        m, outs = C.run_model(make())
        assert all(o is None or isinstance(o, tuple) or o["fits"] for o in outs)
    m, outs = C.run_model(C.second_wave(False))
    assert m.table()[ipv4(C.host(500))][0] == C.mac_of(64) and bytes(m.rows[0]["mac"]) == C.mac_of(63)
    m, outs = C.run_model(C.second_wave(True))
    assert list(outs[0]["action"][:64]) == [R.DROPPED] * 64 and set(m.table()) == {ipv4(C.host(500))}
    m, outs = C.run_model(C.many_waiters())
    order = [(int(y["frame"]), int(y["row"])) for y in outs[0]["ready"]]
    assert order == [(0, 71), (1, 70), (1, 73)] + [(3, r) for r in list(range(70)) + [72]]
