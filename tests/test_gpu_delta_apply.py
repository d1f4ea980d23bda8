"""The deferred control writes on the device: ``Engine.stage_write`` / ``stage_mark_dirty`` /
``stage_unpause`` -> ``DeltaStage::pack_deltas`` -> ``apply_deltas`` (dataplane.hip), against a
byte model of the target buffer.

The model is a numpy ``uint8`` image: every ``stage_write(name, data, offset)`` assigns
``img[offset:offset + n] = data`` in call order (the last write wins).  The targets are named
device buffers of a fresh engine with nothing declared (no kernel touches them): ``tpool`` for
the small cases, ``ring`` for the large ones.  A known random image is uploaded first and the
whole buffer is downloaded afterwards, so a byte written next to a record fails the comparison.

Every case runs on the three paths -- ``flush`` (``flush_deltas()`` between steps: k_apply_deltas)
and ``step`` (empty steps: k_stage carries the records) with and without the captured graph.
The number of applications (kernel launches / steps) a case needs is worked out here from
DELTA_REC_MAX, DELTA_CAP, the dirty cap and the packer's ``need()`` formula, all parsed from the
headers, and the step path must take exactly that many steps; after every step the image must
be the model's image with exactly the records of the applications so far."""

import os
import re

import numpy as np
import pytest

from gpu_cfg import CFG

pytestmark = pytest.mark.gpu

KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "kernels")


def _read(name):
    with open(os.path.join(KERNELS, name)) as f:
        return f.read()


def _limits():
    abi, stage = _read("step_abi.h"), _read("delta_stage.h")
    rec_max = int(re.search(r"#define\s+DELTA_REC_MAX\s+(\d+)", abi).group(1))
    unp_max = int(re.search(r"#define\s+UNPAUSE_STEP_MAX\s+(\d+)", abi).group(1))
    m = re.search(r"DELTA_CAP\s*=\s*(\d+)ull\s*<<\s*(\d+)", stage)
    cap = int(m.group(1)) << int(m.group(2))
    dirty = {int(x) for x in re.findall(r"dirty\.size\(\),\s*(\d+)\)", stage)}
    dirty |= {int(x) for x in re.findall(r"dn\s*<=\s*(\d+)", stage)}
    assert len(dirty) == 1, dirty     # (one cap, used for the first batch and for the later ones)
    # the packer's need(): head + records + padded dirty list + chunks -- as the header states it
    assert "return 16 + 16 * r + ((4 * dn + 15) & ~15ull) + 16 * ch;" in stage
    # and the slack stage_write keeps for one record's head
    assert "if (n + 64 > DELTA_CAP) throw" in stage
    return rec_max, cap, unp_max, dirty.pop()


REC_MAX, CAP, UNP_MAX, DIRTY_MAX = _limits()
PATHS = {"flush": None, "step-graph": True, "step-eager": False}


def need(r, dn, ch):
    return 16 + 16 * r + ((4 * dn + 15) & ~15) + 16 * ch


def chunks(n):
    return (n + 15) // 16


# ---------------------------------------------------------------- the host model
class Batch:
    def __init__(self, open_):
        self.w, self.dirty, self.open = {}, [], open_   # w: offset -> bytes, never overlapping


def cut_in(w, a, data):
    """DeltaStage::stage_write: an earlier write of the batch is cut to what the new one leaves."""
    e = a + len(data)
    for s0 in sorted(w):
        old = w[s0]
        s1 = s0 + len(old)
        if s1 <= a or s0 >= e:
            continue
        del w[s0]
        if s0 < a:
            w[s0] = old[:a - s0]
        if s1 > e:
            w[e] = old[e - s0:]
    w[a] = bytes(data)


def applications(batches):
    """pack_deltas' plan over closed batches, oldest first: [[(offset, bytes)] per application].
    Of the first batch as many records (in address order) as DELTA_REC_MAX and DELTA_CAP allow;
    when it goes whole, the later batches that fit whole and write no byte planned so far."""
    q = [(sorted(b.w.items()), len(b.dirty)) for b in batches if b.w or b.dirty]
    apps = []
    while q:
        w0, d0 = q[0]
        nd0 = min(d0, DIRTY_MAX)
        nrec = nchunk = 0
        for off, data in w0:
            if nrec == REC_MAX or need(nrec + 1, nd0, nchunk + chunks(len(data))) > CAP:
                break
            nrec += 1
            nchunk += chunks(len(data))
        took = list(w0[:nrec])
        assert took or nd0, "a record that fits no step"
        if nrec < len(w0) or nd0 < d0:
            q[0] = (w0[nrec:], d0 - nd0)
        else:
            q.pop(0)
            ndirty = nd0
            while q:
                w, dn = q[0]
                r, ch, ok = nrec, nchunk, ndirty + dn <= DIRTY_MAX
                for off, data in w:
                    r += 1
                    ch += chunks(len(data))
                    ok = ok and r <= REC_MAX and need(r, ndirty + dn, ch) <= CAP and not any(
                        off < o + len(x) and o < off + len(data) for o, x in took)
                if not ok:
                    break
                took += w
                nrec, nchunk, ndirty = r, ch, ndirty + dn
                q.pop(0)
        apps.append(took)
    return apps


class Rig:
    """A fresh engine, a random image in ``target``, and the model beside it."""

    def __init__(self, path, target="tpool", seed=1, **over):
        from chanamq_amd.engine.dataplane import GpuDataPlane
        self.path = path
        self.dp = GpuDataPlane(graph=PATHS[path] is not False, **dict(CFG, **over))
        self.eng, self.target = self.dp.eng, target
        self.size = len(self.eng.download(target))
        self.applied = np.random.default_rng(seed).integers(0, 256, self.size, dtype=np.uint8)
        self.eng.upload(target, self.applied)
        self.img = self.applied.copy()     # last write wins, in call order
        self.batches = []
        self.rng = np.random.default_rng(seed + 1000)

    def _staging(self):
        if not self.batches:
            self.batches.append(Batch(False))
        return self.batches[-1]

    def begin(self):
        self.eng.stage_begin()
        if not self.batches or not self.batches[-1].open:
            self.batches.append(Batch(True))

    def end(self):
        self.eng.stage_end()
        for b in self.batches:
            b.open = False

    def write(self, off, n):
        """n fresh random bytes at ``off``; never closer than 64 bytes to the buffer's end."""
        assert 0 <= off and off + n + 64 <= self.size
        data = self.rng.integers(0, 256, n, dtype=np.uint8)
        self.eng.stage_write(self.target, data, off)
        self.img[off:off + n] = data
        cut_in(self._staging().w, off, data.tobytes())
        return data

    def mark(self, slot):
        self.eng.stage_mark_dirty(slot)
        b = self._staging()
        if slot not in b.dirty:
            b.dirty.append(slot)

    def device(self):
        return np.frombuffer(self.eng.download(self.target), np.uint8)

    def _same(self, want, what):
        got = self.device()
        bad = np.flatnonzero(got != want)
        assert not len(bad), f"{self.path} {what}: {len(bad)} bytes differ, first at {int(bad[0])}"

    def apply(self, expect=None):
        """Apply what is staged; ``expect``: the number of applications the case derived."""
        apps = applications(self.batches)
        if expect is not None:
            assert len(apps) == expect, f"the model plans {len(apps)} applications, the case derived {expect}"
        self.batches = []
        steps = 0
        if self.path == "flush":
            self.eng.flush_deltas()
            for took in apps:
                for off, data in took:
                    self.applied[off:off + len(data)] = np.frombuffer(data, np.uint8)
        else:
            for k, took in enumerate(apps):
                assert self.dp.deltas_pending() != (0, 0, 0), f"nothing pending after {k} of {len(apps)} steps"
                self.dp.step({})
                steps += 1
                for off, data in took:
                    self.applied[off:off + len(data)] = np.frombuffer(data, np.uint8)
                if len(apps) > 1:
                    self._same(self.applied, f"after step {k + 1} of {len(apps)}")
            if len(apps) > 1:
                print(f"{self.path}: {len(apps)} applications derived, {steps} steps taken")
        assert self.dp.deltas_pending() == (0, 0, 0), f"{self.path}: still pending after {len(apps)} applications"
        assert np.array_equal(self.applied, self.img)      # (the two host models agree)
        self._same(self.img, "final image")
        return len(apps)


@pytest.fixture(params=sorted(PATHS))
def path(request, gpu):
    return request.param


# ---------------------------------------------------------------- bytes
LENGTHS = (1, 3, 4, 15, 16, 17, 31, 32, 33)


def test_lengths_and_alignments(path):
    """One record of each length at each ``offset % 4``: the dword path (aligned, a multiple of
    four), the byte path, and a last chunk shorter than 16 bytes on each -- one record per
    application, then all 36 in one."""
    rig = Rig(path)
    spots = [(256 * k + 64 + o, n) for k, (n, o) in enumerate((n, o) for n in LENGTHS for o in range(4))]
    for off, n in spots:
        rig.write(off, n)
        rig.apply(expect=1)
    for off, n in spots:
        rig.write(off + 128, n)
    rig.apply(expect=1)


def test_records_sharing_a_dword_and_a_line(path):
    """Bytes 0..1 and 2..3 of one dword, two records in one 16-byte line, and two that meet
    end to start inside a line: neither clobbers the other (or the bytes between them)."""
    rig = Rig(path)
    rig.write(512, 2)
    rig.write(514, 2)
    rig.write(1024 + 1, 5)
    rig.write(1024 + 8, 8)
    rig.write(2048 + 3, 6)
    rig.write(2048 + 9, 4)
    rig.apply(expect=1)


@pytest.mark.parametrize("layout", ["middle", "first", "last"])
def test_binary_search_edges(path, layout):
    """A 64 KiB record (4096 chunks) among 1-byte records in address order: every chunk finds
    its record -- the first record (lo = 0), the last (lo = nrec - 1), and a record whose
    chunk0 is the batch's last chunk."""
    rig = Rig(path, "ring")
    big = 64 << 10
    assert chunks(big) == 4096
    base = 1 << 20
    if layout == "middle":
        for off in (base - 37, base - 5):
            rig.write(off, 1)
    if layout in ("middle", "first"):
        rig.write(base + 1, big)
        for off in (base + 1 + big + 7, base + big + 300):
            rig.write(off, 1)
    else:
        rig.write(base - 9, 1)
        rig.write(base, big)
    rig.apply(expect=1)


def test_record_limit(path):
    """DELTA_REC_MAX one-byte records at odd addresses go in one application, one more needs
    two -- and exactly one record is left pending after the first step."""
    rig = Rig(path)
    assert need(REC_MAX, 0, REC_MAX) <= CAP       # (the bytes are no limit here: only the record count)
    for k in range(REC_MAX):
        rig.write(65 + 2 * k, 1)
    rig.apply(expect=1)
    for k in range(REC_MAX + 1):
        rig.write(4097 + 2 * k, 1)
    assert rig.dp.deltas_pending() == (REC_MAX + 1, REC_MAX + 1, 0)
    expect = -(-(REC_MAX + 1) // REC_MAX)
    assert expect == 2
    if path != "flush":
        # the first step alone: the records are taken in address order, so the highest is left
        last = 4097 + 2 * REC_MAX
        rig.dp.step({})
        assert rig.dp.deltas_pending() == (1, 1, 0)
        got = rig.device()
        assert got[last] == rig.applied[last] and np.array_equal(np.delete(got, last), np.delete(rig.img, last))
        rig.dp.step({})
        assert rig.dp.deltas_pending() == (0, 0, 0)
        assert np.array_equal(rig.device(), rig.img)
    else:
        rig.apply(expect=expect)


def test_largest_write(path):
    """DELTA_CAP - 64 bytes are accepted and go in one application (head 16 + one record 16 +
    the chunks <= DELTA_CAP); one byte more is refused at stage_write and stages nothing."""
    rig = Rig(path, "ring")
    n = CAP - 64
    assert need(1, 0, chunks(n)) <= CAP < need(1, 0, chunks(n)) + 64
    with pytest.raises(RuntimeError, match="larger than one step"):
        rig.eng.stage_write("ring", np.zeros(n + 1, np.uint8), 4096)
    assert rig.dp.deltas_pending() == (0, 0, 0)
    rig.write(4096 + 3, n)
    assert rig.dp.deltas_pending() == (1, n, 0)
    rig.apply(expect=1)


def test_buffer_overflow_takes_two_applications(path):
    """Two records of 3 MiB each in one batch: either fits a step's buffer, both do not."""
    rig = Rig(path, "ring")
    n = 3 << 20
    assert need(1, 0, chunks(n)) <= CAP < need(2, 0, 2 * chunks(n))
    rig.write(1 << 20, n)
    rig.write((5 << 20) + 2, n)
    assert rig.dp.deltas_pending() == (2, 2 * n, 0)
    rig.apply(expect=2)


def test_overwrites_within_one_batch(path):
    """A, then B over A's middle, then C over B's head: the stager cuts the earlier records,
    one application, the last write of every byte wins."""
    rig = Rig(path)
    rig.write(1000, 100)      # A
    rig.write(1030, 40)       # B
    rig.write(1021, 19)       # C: A's bytes 1021..1029, B's 1030..1039
    assert rig.dp.deltas_pending()[0] == 4       # A's head, C, B's tail, A's tail
    rig.apply(expect=1)
    rig.write(3001, 33)
    rig.write(3001, 33)       # the same bytes again: one record, the second write's
    assert rig.dp.deltas_pending() == (1, 33, 0)
    rig.apply(expect=1)


def test_overwrites_across_batches(path):
    """Two closed sections, the second overwriting bytes of the first: they ride two
    applications (a step's records are applied in parallel), and after the first the image is
    'first batch only'.  Two sections writing disjoint bytes ride one."""
    rig = Rig(path)
    rig.begin()
    rig.write(2000, 64)
    rig.write(3003, 8)
    rig.end()
    rig.begin()
    rig.write(2010, 20)
    rig.write(5000, 4)
    rig.end()
    rig.apply(expect=2)
    rig.begin()
    rig.write(6000, 17)
    rig.end()
    rig.begin()
    rig.write(6017, 15)
    rig.end()
    rig.apply(expect=1)


# ---------------------------------------------------------------- dirty list
def dirty_state(eng):
    flags = np.frombuffer(eng.download("ch_dirty"), np.uint32)
    n = int(np.frombuffer(eng.download("n_dirty"), np.uint32)[0])
    lst = np.frombuffer(eng.download("dirty_list"), np.uint32)[:n]
    return sorted(np.flatnonzero(flags).tolist()), lst.tolist()


def test_dirty_list_flush(gpu):
    """Channel slots marked with no writes at all (1, 3, 4 and 5 of them: the 16-byte padding
    behind the list and nrec == 0), a slot marked twice in a batch and again in a later one, and
    a slot the synchronous path has flagged already: ch_dirty, n_dirty and dirty_list hold every
    marked slot exactly once.  Then marks beside a write: the data behind a padded list of three
    lands where it belongs."""
    rig = Rig("flush")
    eng, want = rig.eng, set()

    def check():
        flags, lst = dirty_state(eng)
        assert flags == sorted(want)
        assert sorted(lst) == sorted(want), f"dirty_list {lst}: every marked slot exactly once"

    for group in ([7], [1, 2, 3], [10, 11, 12, 13], [20, 21, 22, 23, 24]):
        for s in group:
            rig.mark(s)
        assert rig.dp.deltas_pending() == (0, 0, len(group))
        want |= set(group)
        rig.apply(expect=1)
        check()
    rig.mark(30)
    rig.mark(30)
    assert rig.dp.deltas_pending() == (0, 0, 1)
    want.add(30)
    rig.apply(expect=1)
    check()
    rig.mark(30)              # a later batch: the device's flag keeps it off the list
    rig.mark(2)
    rig.apply(expect=1)
    check()
    rig.dp._mark_dirty(40)    # synchronous: flag and list entry uploaded
    want.add(40)
    check()
    rig.mark(40)
    rig.apply(expect=1)
    check()
    for s in (50, 51, 52):    # ndirty 3: the data starts 16 bytes behind the list's start
        rig.mark(s)
    want |= {50, 51, 52}
    rig.write(777, 17)
    rig.apply(expect=1)
    check()


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_dirty_mark_requeues_in_the_carrying_step(gpu, mode):
    """The step path, through its effect: for a channel holding unacked deliveries, ch_req_upto
    and the dirty mark staged in one batch (what channel_closing stages under ``defer``).  Every
    unacked delivery is requeued in the step that carries the batch and delivered again with the
    redelivered flag -- the same bytes and n_requeue as the golden model's channel_closing."""
    from chanamq_amd.engine.dataplane import GpuDataPlane
    from consumer_scenarios import golden_plane, observe, open_ch, pubs, run_consumer
    from dp_scenarios import VH

    def prepare(dp):
        dp.declare_queue(VH, "dq")
        open_ch(dp, 1)
        open_ch(dp, 2)
        dp.consume(2, 1, VH, "dq", "d", no_ack=False)
        return dp

    g = prepare(golden_plane(CFG))
    og = run_consumer(g, [{1: pubs("dq", 0, 5)}])
    g.channel_closing(g.channel(2, 1))
    og += run_consumer(g, [{}, {}])
    d = prepare(GpuDataPlane(graph=mode == "graph", **CFG))
    od = run_consumer(d, [{1: pubs("dq", 0, 5)}])
    s = d.chslot(2, 1)
    d.eng.stage_write("ch_req_upto", np.array([1 << 62], np.uint64), 8 * s)
    d.eng.stage_mark_dirty(s)
    assert d.deltas_pending() == (1, 8, 1)
    od += run_consumer(d, [{}, {}])
    assert d.deltas_pending() == (0, 0, 0)
    assert [o["counters"]["n_requeue"] for o in od[:2]] == [0, 5]
    seen = [x for x in observe(od) if x.step < 2]
    assert [(x.step, x.tag, x.redelivered) for x in seen] == (
        [(0, t, False) for t in range(1, 6)] + [(1, t, True) for t in range(6, 11)])
    assert [o["counters"] for o in og] == [o["counters"] for o in od]
    assert [o["egress"] for o in og] == [o["egress"] for o in od]


# ---------------------------------------------------------------- unpause
def paused(eng):
    return np.frombuffer(eng.download("conn_paused"), np.uint32)


def test_unpause(path):
    """conn_paused set for several connections by upload; stage_unpause clears exactly those
    with the next step (flush_deltas only hands them to it)."""
    rig = Rig(path)
    flags = np.zeros(CFG["c_max"], np.uint32)
    flags[[0, 3, 4, 17, 63]] = 1
    rig.eng.upload("conn_paused", flags)
    for c in (3, 17, 63, 17):
        rig.eng.stage_unpause(c)
    assert rig.dp.deltas_pending() == (0, 0, 0)      # (unpauses are no records)
    if path == "flush":
        rig.eng.flush_deltas()
        assert np.array_equal(paused(rig.eng), flags)
    rig.dp.step({})
    want = flags.copy()
    want[[3, 17, 63]] = 0
    assert np.array_equal(paused(rig.eng), want)
    rig.dp.step({})
    assert np.array_equal(paused(rig.eng), want)


def test_unpause_waits_for_the_writes_staged_before_it(path):
    """An unpause staged behind DELTA_REC_MAX + 1 records: the records need two applications,
    and the connection resumes with the second, not before."""
    rig = Rig(path)
    flags = np.zeros(CFG["c_max"], np.uint32)
    flags[[5, 6]] = 1
    rig.eng.upload("conn_paused", flags)
    for k in range(REC_MAX + 1):
        rig.write(65 + 2 * k, 1)
    rig.eng.stage_unpause(5)
    if path == "flush":
        rig.apply(expect=2)
        assert np.array_equal(paused(rig.eng), flags)       # no step yet
        rig.dp.step({})
    else:
        rig.batches = []
        rig.dp.step({})
        assert rig.dp.deltas_pending() == (1, 1, 0)
        assert np.array_equal(paused(rig.eng), flags), "unpaused before the batch's last records"
        rig.dp.step({})
        assert rig.dp.deltas_pending() == (0, 0, 0)
        assert np.array_equal(rig.device(), rig.img)
    want = flags.copy()
    want[5] = 0
    assert np.array_equal(paused(rig.eng), want)


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_unpause_step_cap(gpu, mode):
    """More connections than one step unpauses (c_max = UNPAUSE_STEP_MAX + 64, the carry cut to
    4 KiB): UNPAUSE_STEP_MAX + 1 unpauses take two steps -- one connection is still paused after
    the first -- and all end cleared; the connections not named stay paused."""
    c_max = UNP_MAX + 64
    rig = Rig("step-" + mode, c_max=c_max, carry_cap=4096)
    flags = np.ones(c_max, np.uint32)
    rig.eng.upload("conn_paused", flags)
    for c in range(UNP_MAX + 1):
        rig.eng.stage_unpause(c)
    assert -(-(UNP_MAX + 1) // UNP_MAX) == 2
    rig.dp.step({})
    assert int(paused(rig.eng)[:UNP_MAX + 1].sum()) == 1
    rig.dp.step({})
    got = paused(rig.eng)
    assert not got[:UNP_MAX + 1].any() and got[UNP_MAX + 1:].all()


# ---------------------------------------------------------------- host-mapped target, refusals
def test_host_mapped_target_is_written_at_once(gpu):
    rig = Rig("flush")
    eng = rig.eng
    before = rig.dp.deltas_pending()
    eng.stage_write("conn_wblock", np.array([0xA5A5A5A5], np.uint32), 4 * 9)
    got = np.frombuffer(eng.download("conn_wblock"), np.uint32)
    assert got[9] == 0xA5A5A5A5 and not np.delete(got, 9).any()
    assert rig.dp.deltas_pending() == before == (0, 0, 0)
    eng.stage_write("conn_wblock", np.array([0], np.uint32), 4 * 9)
    assert not np.frombuffer(eng.download("conn_wblock"), np.uint32).any()


def test_refusals_stage_nothing(gpu):
    """Host-side exceptions raised before anything is staged or launched."""
    rig = Rig("step-graph")
    eng, dp = rig.eng, rig.dp
    nch = CFG["c_max"] * CFG["chpc"]

    def state():
        return dp.deltas_pending(), eng.dl_state(3)

    s0 = state()
    with pytest.raises(RuntimeError, match="overflows"):
        eng.stage_write("tpool", np.zeros(2, np.uint8), rig.size - 1)
    with pytest.raises(RuntimeError, match="no buffer"):
        eng.stage_write("no_such_table", np.zeros(4, np.uint8), 0)
    with pytest.raises(RuntimeError, match="bad channel slot"):
        eng.stage_mark_dirty(nch)
    with pytest.raises(RuntimeError, match="bad connection"):
        eng.stage_unpause(CFG["c_max"])
    assert state() == s0
    # flush_deltas() with a step in flight: refused, and what is staged stays staged
    from chanamq_amd.engine.layout import SEG_IN
    t = dp.submit_raw(np.zeros(0, SEG_IN), dp._pinned(16, 0).ctypes.data, 0)
    rig.write(100, 5)
    s1 = state()
    with pytest.raises(RuntimeError, match="between steps only"):
        eng.flush_deltas()
    assert state() == s1
    dp.finish(t)
    assert np.array_equal(rig.device(), rig.applied)     # nothing applied yet
    rig.apply(expect=1)
