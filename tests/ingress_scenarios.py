"""Ingress-half scenarios in the ``consumer_scenarios`` style: the frame scan (k_frame_scan)
at the places where it changes path -- the join of a connection's carry and its new bytes,
the segment lengths around the LDS stage and the candidate mask, bodies full of frame-header
lookalikes, more frames than candidate slots, more than one emit chunk, the per-step capacity
exits, a connection's own frame-max.  A scenario is ``(dp, lim) -> Run``: it sets up the
control state and returns the steps (``{conn: bytes}``, with ``'__ops__'`` applied before the
step, as in ``consumer_scenarios``) and what every consumer connection must receive.  ``lim``
holds the scan's limits as the built extension exports them (``limits()``).

``check_run`` judges a run from the streams that were sent, never from the golden model:

1. every consumer receives exactly the published bodies, once each, in each publisher's
   order, with delivery tags that count up from 1 on every channel;
2. every segment record accounts for its bytes: consumed + carry = carry before + new bytes
   (a record with SS_TOO_LARGE drops them: carry 0);
3. the kick rule: a carry that begins with a whole command comes with SS_OVERFLOW (the
   native front end re-presents a carry only then), for an unpaused connection without an
   error status -- and no connection gets an error status but the ones the scenario names;
4. progress: a scenario ends with a fixed number of empty steps, worked out from its frames
   and the limits, after which no connection holds a carry and (1) holds.

Scenarios marked ``exact`` are also compared byte by byte with the golden model's run.

The property decode of a publish (k_decode) is judged the same way: ``walk_props`` reads a
property list byte by byte, ``prop_cases`` are lists built to sit on the decode's edges, and
``check_props`` holds a plane's persist records and deliveries to the walk.
"""

import struct
from collections import defaultdict, namedtuple

from chanamq_amd.engine.layout import (SS_CTRL, SS_FRAME_ERROR, SS_OVERFLOW, SS_PAUSED, SS_TOO_LARGE,
                                       SS_UNEXPECTED)
from chanamq_amd.engine.traffic import ack_frame, heartbeat, publish_command
from consumer_scenarios import body_of, observe, open_ch
from dp_scenarios import VH

Scenario = namedtuple("Scenario", "group fn cfg exact")
# steps; {consumer conn: [one publisher's bodies in order, ...]}; the connections that are meant
# to get an error status (no other may), and may end holding bytes
Run = namedtuple("Run", "steps expect errs")
Limits = namedtuple("Limits", "CAND_MAX FS_CAND_STAGED FS_STAGE FS_AM_MAX FS_RUNS")
SS_ERR = SS_FRAME_ERROR | SS_UNEXPECTED | SS_TOO_LARGE


def limits():
    """The frame scan's limits, from the built extension."""
    from chanamq_amd import ops
    m = ops.load()
    return Limits(*(int(getattr(m, k)) for k in Limits._fields))


def staged(L, lim):
    """A segment of L bytes is scanned from the LDS stage (dp_frame_scan.h)."""
    return ((L + 15) >> 4) * 16 + 32 <= lim.FS_STAGE


def cmax(L, lim):
    """Candidate slots of a segment of L bytes."""
    return lim.FS_CAND_STAGED if staged(L, lim) else lim.CAND_MAX


def drain_steps(nframes, L, lim):
    """Empty steps after which a segment of nframes frames must be gone: a step that runs out
    of candidate slots still takes the commands of its first cmax frames, less the at most two
    frames of a publish cut off at the end."""
    return -(-nframes // (cmax(L, lim) - 2)) + 2


# ---------------------------------------------------------------- streams
def exact_stream(n, queue="sq"):
    """Publishes of one connection, exactly n bytes of whole commands."""
    one = lambda size, i: publish_command(1, "", queue, bytes((i * 7 + j) & 0xff for j in range(size)),
                                          {"delivery_mode": 1})
    ovh = len(one(1, 0)) - 1
    out, total, i = [], 0, 0
    while n - total > 2 * (ovh + 1000):
        out.append(one(1000, i))
        total += len(out[-1])
        i += 1
    rest = n - total - ovh
    if rest > 1200:   # (two commands: neither body empty)
        out.append(one(rest // 2 - ovh, i))
        total += len(out[-1])
        rest = n - total - ovh
    assert rest >= 1
    out.append(one(rest, i + 1))
    data = b"".join(out)
    assert len(data) == n
    return data


def frames(data):
    pos = 0
    while pos < len(data):
        end = pos + 8 + int.from_bytes(data[pos + 3:pos + 7], "big")
        yield pos, end
        pos = end


def commands(data):
    """(start, end, body or None, frames) of every whole command from the front of a stream
    the test built itself (well formed): a heartbeat, a method frame, or a publish with its
    header and body frames.  Stops at the first command that is not all there."""
    pos, n = 0, len(data)

    def frame(p):
        if p + 8 > n:
            return None
        t, _, size = struct.unpack_from(">BHI", data, p)
        return (t, p + 8 + size) if p + 8 + size <= n else None

    while True:
        f = frame(pos)
        if f is None:
            return
        t, end = f
        if t != 1 or struct.unpack_from(">HH", data, pos + 7) != (60, 40):
            yield pos, end, None, 1
            pos = end
            continue
        h = frame(end)
        if h is None:
            return
        bsz = struct.unpack_from(">Q", data, end + 7 + 4)[0]
        e, got, parts = h[1], 0, []
        while got < bsz:
            b = frame(e)
            if b is None:
                return
            parts.append(data[e + 7:b[1] - 1])
            got += len(parts[-1])
            e = b[1]
        yield pos, e, b"".join(parts), 2 + len(parts)
        pos = e


def bodies_of(data):
    return [c[2] for c in commands(data) if c[2] is not None]


def nframes(data):
    return sum(1 for _ in frames(data))


def pub(key, body, ch=1, fm=131072, props=None):
    return publish_command(ch, "", key, body, props, frame_max=fm)


def sent_by(steps, conn):
    return b"".join(s.get(conn, b"") for s in steps)


def pubsub(dp, queues=("iq",), pub_fm=None):
    """Connection 1 publishes; connection 2 consumes every queue, auto-ack, on channel 1."""
    for q in queues:
        dp.declare_queue(VH, q)
    open_ch(dp, 1, frame_max=pub_fm)
    open_ch(dp, 2)
    for q in queues:
        dp.consume(2, 1, VH, q, "c-" + q, no_ack=True)


def one_publisher(steps, errs=()):
    return Run(steps, {2: [bodies_of(sent_by(steps, 1))]}, frozenset(errs))


# ---------------------------------------------------------------- A: carry joins new bytes
JOIN_BIG = 60_000


def sc_join(dp, lim):
    """Two publishes (a 1-byte key, a 33-byte body; then one more), cut at every byte of the
    first command: carries of every length mod 16, the cut inside each of the 7 header bytes
    of the method, header and body frame, on each end marker and exactly between two frames.
    Then a publish whose 60,000-byte body frame straddles: the carry is the method, the header
    and 5 bytes of the body frame."""
    pubsub(dp, ("j",))
    steps, i = [], 0
    first = pub("j", body_of("j", 0, 33))
    for k in range(1, len(first)):
        s = pub("j", body_of("j", i, 33)) + pub("j", body_of("j", i + 1, 20))
        assert len(pub("j", body_of("j", i, 33))) == len(first)
        i += 2
        steps += [{1: s[:k]}, {1: s[k:]}, {}]
    big = pub("j", body_of("j", i, JOIN_BIG))
    fr = list(frames(big))
    assert len(fr) == 3 and fr[2][1] - fr[2][0] == JOIN_BIG + 8
    k = fr[2][0] + 5
    steps += [{1: big[:k]}, {1: big[k:]}, {}]
    return one_publisher(steps)


# ---------------------------------------------------------------- B: segment lengths
CARRY = 37


def sc_lengths(dp, lim):
    """Segments of exactly L bytes, each without a carry (scanned in place) and behind a
    37-byte carry left by the step before (fused or split, an odd residue): the last staged
    and the first unstaged length, the last and the first around the candidate mask's size.
    Then the ends: a lone heartbeat cut after 1..7 bytes -- a partial header only, then a
    whole header without its end marker -- and whole, alone and at the end of a segment that
    began in the carry."""
    pubsub(dp, ("sq",))
    last_staged = lim.FS_STAGE - 32
    assert staged(last_staged, lim) and not staged(last_staged + 1, lim)
    steps = []
    for L in (last_staged, last_staged + 1, lim.FS_AM_MAX * 16, lim.FS_AM_MAX * 16 + 1):
        s = exact_stream(L)
        steps += [{1: s}, {1: s[:CARRY]}, {1: s[CARRY:]}]
    hb = heartbeat()
    for n in range(1, 9):
        p = pub("sq", body_of("sq", n, 50))
        steps += [{1: hb[:n]}, {1: hb[n:]}, {1: p[:CARRY]}, {1: p[CARRY:] + hb[:n]}, {1: hb[n:]}]
    return one_publisher([s for s in steps if s[1]] + [{}])


# ---------------------------------------------------------------- C: header lookalikes
LOOK9 = bytes.fromhex("08000000000000ceff")   # a whole "heartbeat"; what follows is no header
LOOK8 = bytes.fromhex("08000000000000ce")     # a whole "heartbeat"; the next one follows it
RAW8 = bytes.fromhex("0100000000000000")      # passes the screen; no end marker, ends inside
ONES = bytes.fromhex("00000001")              # type 1, channel 0, size 65536: runs past the end


def lookalike(dp, lim, stream, pub_fm=None, model_free=False):
    pubsub(dp, ("lq",), pub_fm=pub_fm)
    n = drain_steps(nframes(stream), len(stream), lim) if model_free else 1
    return one_publisher([{1: stream}] + [{}] * n)


def sc_look_failures(dp, lim):
    """300 whole lookalikes over 10 publishes, each followed by a byte that starts nothing:
    300 chain failures with a broken successor, jumped over by the run records."""
    return lookalike(dp, lim, b"".join(pub("lq", body_of("lq", i) + LOOK9 * 30) for i in range(10)))


def sc_look_runs(dp, lim):
    """FS_RUNS + 1 small publishes with one lookalike each: more runs than run records, so
    one thread walks the chain."""
    return lookalike(dp, lim, b"".join(pub("lq", body_of("lq", i) + LOOK9) for i in range(lim.FS_RUNS + 1)))


def sc_look_fail_max(dp, lim):
    """One body of more lookalikes than the failure list holds (cmax - 2 FS_RUNS), fewer than
    cmax: the other trigger of the serial walk."""
    n = lim.FS_CAND_STAGED - 2 * lim.FS_RUNS + 104
    s = pub("lq", body_of("lq", 0) + LOOK9 * n) + pub("lq", body_of("lq", 1))
    assert n + nframes(s) < lim.FS_CAND_STAGED and staged(len(s), lim)
    return lookalike(dp, lim, s)


def sc_look_raw(dp, lim):
    """More raw candidates than slots, none of them accepted: every thread validates its own
    words against the mask."""
    s = pub("lq", body_of("lq", 0) + RAW8 * (lim.FS_CAND_STAGED + 56)) + pub("lq", body_of("lq", 1))
    assert staged(len(s), lim)
    return lookalike(dp, lim, s)


def sc_look_past_end(dp, lim):
    """The segment's last command is 20,000 bytes of big-endian ones: 5,000 accepted
    lookalikes, each a frame that runs past the end of the segment."""
    s = pub("lq", body_of("lq", 0, 40)) + pub("lq", ONES * 5000)
    assert 5000 + nframes(s) < lim.FS_CAND_STAGED
    return lookalike(dp, lim, s)


def sc_look_over_ones(dp, lim):
    """60,048 bytes of big-endian ones in one body: every one of the 15,012 reads as a frame
    that runs past the segment and is accepted, more than the candidate list holds; three
    small publishes behind them."""
    s = pub("lq", ONES * 15012) + b"".join(pub("lq", body_of("lq", i, 30)) for i in range(3))
    assert staged(len(s), lim) and len(candidates(s)) > 15012 > lim.FS_CAND_STAGED
    return lookalike(dp, lim, s, model_free=True)


def sc_look_over_fm32k(dp, lim):
    """A 70,000-byte body on a frame-max 32768 connection, its front filled with more chained
    lookalikes than a staged segment has slots: the third body frame lies beyond the cut."""
    n = lim.FS_CAND_STAGED + 56
    body = (LOOK8 * n).ljust(70_000, b"\xaa")
    s = pub("lq", body, fm=32768)
    fr = list(frames(s))
    assert staged(len(s), lim) and len(fr) == 5 and fr[4][0] > fr[2][0] + 7 + 8 * lim.FS_CAND_STAGED
    return lookalike(dp, lim, s, pub_fm=32768, model_free=True)


def sc_look_over_unstaged(dp, lim):
    """A 140,000-byte body of big-endian ones in two body frames (frame-max 131072): an
    unstaged segment, the second body frame beyond the cut of the candidate list."""
    s = pub("lq", ONES * 35_000)
    fr = list(frames(s))
    first = len(s) - 65_544   # lookalikes from here on run past the end: accepted
    assert len(fr) == 4 and len(s) > lim.FS_AM_MAX * 16 and (fr[3][0] - first) // 4 > lim.CAND_MAX
    return lookalike(dp, lim, s, model_free=True)


# ---------------------------------------------------------------- D: more frames than slots
def flood(groups, lead=0):
    """``lead`` heartbeats, then ``groups`` times 124 heartbeats and a 1-byte-body publish."""
    return heartbeat() * lead + b"".join(heartbeat() * 124 + pub("d", bytes([i & 0xff])) for i in range(groups))


def candidates(data, fmax=131072):
    """The positions the scan's phase (a) accepts in a segment, by its own rule: a frame type,
    a size within the frame-max, and either the end marker in place or a frame that runs past
    the end of the segment; then the positions too close to the end for a whole header."""
    L, out = len(data), []
    for p in range(max(L - 6, 0)):
        if data[p] in (1, 2, 3, 8):
            size = int.from_bytes(data[p + 3:p + 7], "big")
            if size + 8 <= fmax and (p + 8 + size > L or data[p + 7 + size] == 0xCE):
                out.append(p)
    return out + list(range(max(L - 6, 0), L))


def cut_leads(s, last, kinds=(1,)):
    """How many heartbeats in front of the flood ``s`` make the position in slot ``last`` of
    the list a frame of each type in ``kinds`` (1 method, 2 header) -- first for the list of
    accepted candidates, then for a list of the frames alone.  (Heartbeats in front move every
    position and the segment's end alike: the list behind them is the same list.)"""
    starts = {a for a, _ in frames(s)}
    out = []
    for listed in (candidates(s), sorted(starts)):
        assert len(listed) > last + 2
        for kind in kinds:
            out.append(next(n for n in range(256) if listed[last - n] in starts and s[listed[last - n]] == kind))
    return out


def sc_flood_staged(dp, lim):
    """6,350 frames in 52,050 bytes, more than a staged segment's slots.  As it is; then
    behind as many heartbeats as make the last candidate the list holds a publish's method
    frame, then its header frame -- a chain cut inside a command.  The candidates are the
    frames and one lookalike in every body frame (its channel's low byte, 01, reads as a type
    with the bytes after it as a size that runs past the segment); the same two cuts again
    counted in frames alone, for a scan that lists nothing but frames."""
    pubsub(dp, ("d",))
    s = flood(50)
    assert len(s) == 52_050 and nframes(s) == 6350 > lim.FS_CAND_STAGED and staged(len(s) + 8 * 128, lim)
    steps = []
    for lead in [0] + cut_leads(s, lim.FS_CAND_STAGED - 1, (1, 2)):
        f = flood(50, lead)
        steps += [{1: f}] + [{}] * drain_steps(nframes(f), len(f), lim)
    return one_publisher(steps)


def sc_flood_unstaged(dp, lim):
    """The same pattern, more than CAND_MAX frames in a segment too long for the stage."""
    pubsub(dp, ("d",))
    groups = 1
    while nframes(flood(groups)) <= lim.CAND_MAX or staged(len(flood(groups)), lim):
        groups += 1
    steps = []
    for lead in [0] + cut_leads(flood(groups), lim.CAND_MAX - 1):
        f = flood(groups, lead)
        assert len(f) <= lim.FS_AM_MAX * 16 and not staged(len(f), lim)
        steps += [{1: f}] + [{}] * drain_steps(nframes(f), len(f), lim)
    return one_publisher(steps)


# ---------------------------------------------------------------- E: several emit chunks
ACK_CH = 8


def sc_chunk_pubs(dp, lim):
    """1,100 publishes with 1-byte bodies (3,300 frames, four emit chunks of 1,024): a method
    frame is frame 1023, its header frame 1024; publish ordinals run on over the chunks."""
    pubsub(dp, ("d",))
    s = b"".join(pub("d", bytes([i % 251])) for i in range(1100))
    assert len(s) == 53_900 and nframes(s) == 3300
    return one_publisher([{1: s}, {}, {}])


def acks_n(n, lead=0):
    """One consumer connection, 8 channels, a manual-ack consumer on a queue of its own on
    each.  It holds ``held`` deliveries and settles n of them with single acks in one segment,
    round-robin over the channels, behind ``lead`` heartbeats; the rest in the next step.  The
    connection is then closed and a fresh consumer attaches to every queue: an ack that was
    lost comes back to it, flagged."""
    held = 1100 if n <= 1100 else n + 52

    def sc(dp, lim):
        qs = [f"a{c}" for c in range(ACK_CH)]
        for q in qs:
            dp.declare_queue(VH, q)
        open_ch(dp, 1)
        open_ch(dp, 2, *range(1, ACK_CH + 1))
        for c, q in enumerate(qs):
            dp.consume(2, c + 1, VH, q, "m-" + q, no_ack=False)
        msgs = [(qs[i % ACK_CH], body_of(qs[i % ACK_CH], i // ACK_CH)) for i in range(held)]
        ack = [ack_frame(j % ACK_CH + 1, j // ACK_CH + 1, multiple=False) for j in range(held)]
        fresh = [("close_connection", (2,)), ("open_connection", (3, VH)), ("open_channel", (3, 1))]
        fresh += [("consume", (3, 1, VH, q, "f-" + q), dict(no_ack=True)) for q in qs]
        half = held // 2
        steps = [{1: b"".join(pub(q, b) for q, b in msgs[:half])}, {1: b"".join(pub(q, b) for q, b in msgs[half:])},
                 {2: heartbeat() * lead + b"".join(ack[:n])}, {2: b"".join(ack[n:])}, {},
                 {"__ops__": fresh}, {}]
        return Run(steps, {2: [[b for q, b in msgs if q == qq] for qq in qs], 3: [[]]}, frozenset())
    sc.__doc__ = acks_n.__doc__
    return sc


# ---------------------------------------------------------------- F: per-step capacity exits
CMD_MAX = 1024   # the engine sets no floor; 1024 is the smallest any of the project's configurations uses


def two_publishers(dp, fm=None):
    for q in ("fa", "fb"):
        dp.declare_queue(VH, q)
    open_ch(dp, 1, frame_max=fm)
    open_ch(dp, 3, frame_max=fm)
    open_ch(dp, 2, 1, 2)
    dp.consume(2, 1, VH, "fa", "c-fa", no_ack=True)
    dp.consume(2, 2, VH, "fb", "c-fb", no_ack=True)


def capacity_run(a, b):
    n = len(list(commands(a))) + len(list(commands(b)))
    steps = [{1: a, 3: b}] + [{}] * (-(-n // CMD_MAX) + 2)
    return Run(steps, {2: [bodies_of(a), bodies_of(b)]}, frozenset())


def sc_cmd_max(dp, lim):
    """Two publishers, 700 commands each: either fits cmd_max = 1024, both do not.  Whichever
    segment reserves second is carried whole and flagged."""
    two_publishers(dp)
    a = b"".join(pub("fa", body_of("fa", i)) for i in range(700))
    b = b"".join(pub("fb", body_of("fb", i)) for i in range(700))
    return capacity_run(a, b)


FRAG_MAX = 64
FRAG_FM = 4096


def sc_frag_max(dp, lim):
    """Two frame-max 4096 publishers, 8 publishes of 6 body frames each: 48 fragments fit
    frag_max = 64, 96 do not."""
    two_publishers(dp, fm=FRAG_FM)
    size = 5 * (FRAG_FM - 8) + 100
    a = b"".join(pub("fa", body_of("fa", i, size), fm=FRAG_FM) for i in range(8))
    b = b"".join(pub("fb", body_of("fb", i, size), fm=FRAG_FM) for i in range(8))
    assert nframes(a) == 8 * 8
    return capacity_run(a, b)


SMALL_CARRY = 4096


def sc_carry_too_large(dp, lim):
    """carry_cap 4096 and the first 5,007 bytes of a 6,000-byte method frame: nothing can be
    consumed and the rest does not fit the carry -- SS_TOO_LARGE, carry 0, the bytes dropped.
    The other publisher is served in that step; once the connection is closed and opened
    again, both are."""
    two_publishers(dp)
    part = struct.pack(">BHI", 1, 0, 6000) + struct.pack(">HH", 50, 10) + b"\x00" * 4996
    a = b"".join(pub("fa", body_of("fa", i)) for i in range(5))
    b = [b"".join(pub("fb", body_of("fb", i)) for i in r) for r in (range(0, 5), range(5, 10))]
    again = [("close_connection", (1,)), ("open_connection", (1, VH)), ("open_channel", (1, 1))]
    steps = [{1: part, 3: b[0]}, {"__ops__": again, 1: a, 3: b[1]}, {}]
    return Run(steps, {2: [bodies_of(a), bodies_of(b[0] + b[1])]}, frozenset({1}))


# ---------------------------------------------------------------- G: a connection's frame-max
def sc_frame_max(dp, lim):
    """A frame-max 4096 publisher: body frames of fm - 8 bytes are taken; a frame of fm - 7
    passes the screen (the broker's limit is 131072) and fails the connection's own limit:
    SS_FRAME_ERROR at that frame."""
    pubsub(dp, ("gq",), pub_fm=FRAG_FM)
    ok = pub("gq", body_of("gq", 0, 2 * (FRAG_FM - 8)), fm=FRAG_FM)
    assert [e - s for s, e in frames(ok)][2:] == [FRAG_FM, FRAG_FM]
    bad = struct.pack(">BHI", 3, 1, FRAG_FM - 7) + b"\x55" * (FRAG_FM - 7) + b"\xce"
    return Run([{1: ok + bad}, {}], {2: [bodies_of(ok)]}, frozenset({1}))


def frame_max_record(run):
    """The publisher's segment record of the first step: everything up to the long frame is
    consumed, the frame itself stays."""
    data = run.steps[0][1]
    ok = next(commands(data))[1]
    return (1, SS_FRAME_ERROR, ok, len(data) - ok)


BIG = dict(ucap=2048)
SCENARIOS = {
    "join": Scenario("A", sc_join, {}, True),
    "lengths": Scenario("B", sc_lengths, {}, True),
    "look_failures": Scenario("C", sc_look_failures, {}, True),
    "look_runs": Scenario("C", sc_look_runs, BIG, True),
    "look_fail_max": Scenario("C", sc_look_fail_max, {}, True),
    "look_raw": Scenario("C", sc_look_raw, {}, True),
    "look_past_end": Scenario("C", sc_look_past_end, {}, True),
    "look_over_ones": Scenario("C", sc_look_over_ones, {}, False),
    "look_over_fm32k": Scenario("C", sc_look_over_fm32k, {}, False),
    "look_over_unstaged": Scenario("C", sc_look_over_unstaged, {}, False),
    "flood_staged": Scenario("D", sc_flood_staged, BIG, False),
    "flood_unstaged": Scenario("D", sc_flood_unstaged, BIG, False),
    "chunk_pubs": Scenario("E", sc_chunk_pubs, BIG, True),
    "acks_1023": Scenario("E", acks_n(1023), BIG, True),
    "acks_1024": Scenario("E", acks_n(1024), BIG, True),
    "acks_1025": Scenario("E", acks_n(1025), BIG, True),
    "acks_2048": Scenario("E", acks_n(2048), BIG, True),
    "acks_1024_heartbeat": Scenario("E", acks_n(1024, lead=1), BIG, True),
    "cmd_max": Scenario("F", sc_cmd_max, dict(BIG, cmd_max=CMD_MAX), False),
    "frag_max": Scenario("F", sc_frag_max, dict(cmd_max=CMD_MAX, frag_max=FRAG_MAX), False),
    "carry_too_large": Scenario("F", sc_carry_too_large, dict(carry_cap=SMALL_CARRY), False),
    "frame_max": Scenario("G", sc_frame_max, {}, True),
}


# ---------------------------------------------------------------- H: property decode
# (not in SCENARIOS: judged by a property walk of the test's own, see walk_props)
NON_ASCII_DIGITS = "\u0661\u0662"   # ARABIC-INDIC DIGIT ONE, TWO: str.isdigit() takes them, the broker does not
EXPIRATIONS = ["", "0", "00012", "12a", "-1", " 5", "0" * 16 + "12", "0" * 17 + "12", NON_ASCII_DIGITS]
PROP_STEP_MS = 3000
PROP_CFG = dict(persist=1, persist_max=4096, persist_bytes=8 << 20)


def raw_publish(key, raw_props, body, ch=1):
    """A publish whose property list is given as bytes (flags words and values)."""
    from chanamq_amd.protocol.codec import Method, encode_frame, encode_method_frame
    m = Method("basic.publish", exchange="", routing_key=key, mandatory=False)
    return (encode_method_frame(ch, m) + encode_frame(2, ch, struct.pack(">HHQ", 60, 0, len(body)) + raw_props)
            + encode_frame(3, ch, body))


def prop_cases():
    """[(name, queue, raw property list)].  The expiration strings go to a queue of their own
    each ("he<i>": a message expires only at the head of its queue); the rest to "hd", none
    of them with an expiration that runs out within the test."""
    from chanamq_amd.protocol.codec import encode_properties as enc
    cases = [(f"expiration {e!r}", f"he{i}", enc({"delivery_mode": 2, "expiration": e}))
             for i, e in enumerate(EXPIRATIONS)]
    for n in range(18, 35):   # delivery_mode, expiration and timestamp move across byte 32 of the list
        cases.append((f"content_type {n}", "hd", enc({"content_type": "t" * n, "delivery_mode": 2,
                                                      "expiration": f"4{n:04d}", "timestamp": 1_700_000_000 + n})))
    full = {name: "s" * 255 for name, kind in _props() if kind == "shortstr"}
    full.update(headers={f"k{i:02d}": "v" * 56 for i in range(16)}, delivery_mode=2, priority=7, expiration="123456",
                timestamp=1_700_000_099)
    cases.append(("all 14 properties", "hd", enc(full)))
    assert len(enc({"headers": full["headers"]})) > 1024 and len(full) == 14
    # a continuation flags word: delivery_mode and expiration in the first, nothing in the second
    cases.append(("continuation word", "hd", struct.pack(">HH", (1 << 12) | (1 << 8) | 1, 0) + b"\x02" + b"\x0540000"))
    # delivery_mode 2 and an expiration ahead of a message_id cut short: no property counts
    cases.append(("truncated list", "hd", struct.pack(">H", (1 << 12) | (1 << 8) | (1 << 7)) + b"\x02" + b"\x0212"
                  + b"\x09abc"))
    # the continuation bit promises a second flags word; one value byte follows instead
    cases.append(("truncated continuation", "hd", struct.pack(">H", (1 << 12) | 1) + b"\x02"))
    return cases


def _props():
    from chanamq_amd.protocol.codec import BASIC_PROPERTIES
    return BASIC_PROPERTIES


def walk_props(raw):
    """The plain reading of a property list, byte by byte: (persistent, expiration in ms or
    None, timestamp in s or None).  The first flags word names the fields, continuation words
    are skipped; an expiration counts when it is 1 to 18 ASCII digits; a list that ends
    inside a flags word or a field has no properties at all (the reference broker never gets
    a content header out of one: its decoder throws)."""
    none = (False, None, None)
    pos, flags = 0, None
    while True:
        if pos + 2 > len(raw):
            return none
        w = (raw[pos] << 8) | raw[pos + 1]
        pos += 2
        flags = w if flags is None else flags
        if not w & 1:
            break
    persistent, expiration, timestamp = none
    for bit in range(15, 1, -1):
        if not flags & (1 << bit):
            continue
        if bit == 13:      # headers: a table behind its 32-bit length
            if pos + 4 > len(raw):
                return none
            n = 4 + int.from_bytes(raw[pos:pos + 4], "big")
        elif bit in (12, 11):
            n = 1
        elif bit == 6:
            n = 8
        else:              # a short string behind its length octet
            if pos + 1 > len(raw):
                return none
            n = 1 + raw[pos]
        if pos + n > len(raw):
            return none
        field = raw[pos:pos + n]
        pos += n
        if bit == 12:
            persistent = field[0] == 2
        elif bit == 8:
            digits = field[1:]
            if 1 <= len(digits) <= 18 and all(0x30 <= c <= 0x39 for c in digits):
                expiration = int(digits.decode("ascii"))
        elif bit == 6:
            timestamp = int.from_bytes(field, "big")
    return persistent, expiration, timestamp


def run_props(dp, now):
    """Publish every case at ``now``; attach a consumer to every queue; step again at now +
    PROP_STEP_MS.  -> (cases with their bodies, the first step's persist records, outs)."""
    cases = [(name, q, raw, b"%02d:" % i + name.encode("ascii", "replace")) for i, (name, q, raw) in enumerate(prop_cases())]
    queues = sorted({q for _, q, _, _ in cases})
    for q in queues:
        dp.declare_queue(VH, q, durable=True)
    open_ch(dp, 1)
    data = b"".join(raw_publish(q, raw, body) for _, q, raw, body in cases)
    r0 = dp.step({1: data}, now_ms=now)
    records = dp.take_persist()
    open_ch(dp, 2)
    for q in queues:
        dp.consume(2, 1, VH, q, "c-" + q, no_ack=True)
    r1 = dp.step({}, now_ms=now + PROP_STEP_MS)
    eg = [r["egress"] if isinstance(r, dict) else r.egress for r in (r0, r1)]
    segs = [[tuple(s[:4]) for s in (r["segs"] if isinstance(r, dict) else r.segs)] for r in (r0, r1)]
    return cases, records, [dict(egress=e, segs=s) for e, s in zip(eg, segs)]


def delivered_bodies(outs):
    """Bodies of every content command in the egress, properties unread (``observe`` decodes
    them, and some of these lists are cut short on purpose)."""
    out = []
    for o in outs:
        for conn in sorted(o["egress"]):
            data, want, parts = o["egress"][conn], None, []
            for a, b in frames(data):
                if data[a] == 2:
                    want, parts = struct.unpack_from(">Q", data, a + 7 + 4)[0], []
                elif data[a] == 3:
                    parts.append(data[a + 7:b - 1])
                if want is not None and sum(map(len, parts)) >= want:
                    out.append(b"".join(parts))
                    want = None
    return out


def check_props(dp, cases, records, outs, now):
    """Every case against walk_props: a persist record exactly for the persistent ones, with
    the walk's expiry and timestamp; delivered at now + PROP_STEP_MS exactly when not expired."""
    slot = {dp.queues[(VH, q)].slot: q for q in {q for _, q, _, _ in cases}}
    by_body = {r[8]: r for r in records}
    assert len(by_body) == len(records)
    delivered = set(delivered_bodies(outs))
    for name, q, raw, body in cases:
        persistent, exp, ts = walk_props(raw)
        rec = by_body.get(body)
        assert (rec is not None) == persistent, f"{name}: persist record {rec is not None}, delivery_mode says {persistent}"
        if rec is not None:
            assert slot[rec[2]] == q and rec[7] == raw, name
            assert rec[4] == (0 if exp is None else now + exp), f"{name}: expire_ms {rec[4] - now if rec[4] else 0} after now"
            if ts is not None:
                assert rec[1] == ts * 1000, f"{name}: ts_ms {rec[1]}"
        alive = exp is None or exp > PROP_STEP_MS
        assert alive or q != "hd"
        assert (body in delivered) == alive, f"{name}: delivered {body in delivered}, expected {alive}"
    assert len(delivered) == len(delivered_bodies(outs))


# ---------------------------------------------------------------- the model-free checks
def whole_command_at(buf):
    return next(commands(buf), None) is not None


def check_deliveries(outs, expect):
    """(1) each consumer connection got its publishers' bodies, once each, in each
    publisher's order; tags count up from 1 per channel; nothing is flagged redelivered."""
    seen = [s for s in observe(outs) if s.kind == "deliver"]
    nxt = defaultdict(lambda: 1)
    for s in seen:
        assert s.tag == nxt[(s.conn, s.ch)], f"step {s.step} channel {(s.conn, s.ch)}: tag {s.tag}"
        nxt[(s.conn, s.ch)] += 1
        assert not s.redelivered, f"step {s.step} conn {s.conn}: {s.body[:16]!r} redelivered"
    assert {s.conn for s in seen} <= set(expect)
    for conn, lists in expect.items():
        got = [s.body for s in seen if s.conn == conn]
        if len(lists) == 1:
            want = lists[0]
            assert len(got) == len(want), f"conn {conn}: {len(got)} deliveries of {len(want)}"
            bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
            assert not bad, f"conn {conn}: delivery {bad[0]} is not publish {bad[0]}"
            continue
        every = [b for one in lists for b in one]
        assert len(set(every)) == len(every)
        assert sorted(got) == sorted(every), f"conn {conn}: {len(got)} deliveries of {len(every)}, or not those"
        for one in lists:
            mine = set(one)
            assert [b for b in got if b in mine] == one, f"conn {conn}: a publisher's order changed"


def check_segments(steps, outs, errs=frozenset()):
    """(2) the bytes add up, (3) the kick rule, (4) nothing is left in a carry at the end; and
    no connection gets an error status but those in ``errs``."""
    sent = defaultdict(bytes)      # the connection's stream since it was opened
    base = defaultdict(int)        # bytes of it consumed (or dropped) so far
    carry = defaultdict(int)
    paused = set()
    for k, (inp, o) in enumerate(zip(steps, outs)):
        for op in inp.get("__ops__", []):
            if op[0] in ("close_connection", "open_connection"):
                c = op[1][0]
                sent[c], base[c], carry[c] = b"", 0, 0
                paused.discard(c)
        paused -= set(inp.get("__unpause__", []))
        recs = {s[0]: s[1:] for s in o["segs"]}
        assert len(recs) == len(o["segs"])
        for c, data in inp.items():
            if isinstance(c, int):
                assert c in recs or not data, f"step {k}: no segment record for conn {c}"
                sent[c] += data
        for c, (status, consumed, left) in recs.items():
            new = len(inp.get(c, b""))
            assert not status & SS_ERR or c in errs, f"step {k} conn {c}: status {status:#x} on a well-formed stream"
            if status & SS_TOO_LARGE:
                assert left == 0, f"step {k} conn {c}: SS_TOO_LARGE with carry {left}"
                base[c], carry[c] = len(sent[c]), 0
                continue
            assert consumed + left == carry[c] + new, (
                f"step {k} conn {c}: consumed {consumed} + carry {left} != carry before {carry[c]} + new {new}")
            base[c] += consumed
            carry[c] = left
            if status & SS_CTRL:
                paused.add(c)
            if status & (SS_ERR | SS_PAUSED) or c in paused:
                continue
            if whole_command_at(sent[c][base[c]:]):
                assert status & SS_OVERFLOW, (
                    f"step {k} conn {c}: a whole command waits in the carry ({left} bytes) without SS_OVERFLOW")
    left = {c: n for c, n in carry.items() if n and c not in errs}
    assert not left, f"carries left after the last step: {left}"


def check_run(run, outs):
    check_deliveries(outs, run.expect)
    check_segments(run.steps, outs, run.errs)
