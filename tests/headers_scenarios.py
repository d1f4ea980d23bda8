"""Headers exchanges matched on their bindings' arguments (``headers_match=True``: the headers
branch of route_one, csrc/kernels/dp_headers.h, and the golden model's use of
``models/matcher.py``) -- at the places where the matcher changes path, in the style of
``route_scenarios``.

A scenario is ``(dp, lim) -> Run``.  It declares its topology through an ``HWorld``
(``route_scenarios.World`` plus bindings with arguments, exchange-to-exchange edges and
publishes with headers), which keeps its own record and works out the queues of every publish
with ``brute_match`` below: a matcher of this file's own, written over Python dicts and lists
-- never ``models/matcher.py``, which is the golden side's, nor the golden model.  The runs are
judged by ``route_scenarios.check_run``.  ``lim`` holds the limits the built extension exports
(``limits()``); table capacities come from the plane (``dp.hb_max``, ``dp.hp_max``).
"""

import inspect
import struct
from collections import defaultdict, namedtuple
from decimal import Decimal

from chanamq_amd.engine.control import ControlError
from chanamq_amd.protocol.codec import Method, Typed, encode_frame, encode_table
from dp_scenarios import VH
from route_scenarios import CHUNK, Pub, Scenario, World, body_of, bulk, is_golden, topic_hit

Limits = namedtuple("Limits", "HB_PAIRS PUB_QC")
HCFG = dict(hb_max=64, hp_max=256)


def limits():
    from chanamq_amd import ops
    m = ops.load()
    return Limits(*(int(getattr(m, k)) for k in Limits._fields))


def golden_plane(cfg, headers_match=True):
    """The golden model with the engine config ``cfg`` and the device's table bounds."""
    from chanamq_amd.engine.golden import GoldenDataPlane
    from consumer_scenarios import GOLDEN_KEYS
    kw = {k: cfg[k] for k in GOLDEN_KEYS + ("hash_wildcard", "ring_pool", "deliv_max", "egress_cap") if k in cfg}
    if headers_match:
        kw["headers_match"] = True
    g = GoldenDataPlane(**kw)
    if headers_match:
        g.hb_max, g.hp_max, g.hb_pairs = cfg.get("hb_max"), cfg.get("hp_max"), limits().HB_PAIRS
    return g


def fnv32(b):
    h = 0x811C9DC5
    for c in b:
        h = ((h ^ c) * 0x01000193) & 0xFFFFFFFF
    return h


# ---------------------------------------------------------------- the brute-force matcher
SIGNED = {"b": 8, "s": 16, "I": 32, "l": 64, "T": 64}      # 'T' is read as a signed 64-bit value
UNSIGNED = {"B": 8, "u": 16, "i": 32}


def text_of(v):
    """What a field value compares as: ("text", bytes) for strings, booleans, void and every
    integer (its decimal text), ("raw", tag, wire bytes) for floats, decimals, arrays, tables."""
    if isinstance(v, Typed):
        if v.tag in SIGNED or v.tag in UNSIGNED:
            n = int(v.value)
            if v.tag in SIGNED and n >= 1 << (SIGNED[v.tag] - 1):
                n -= 1 << SIGNED[v.tag]
            return "text", str(n).encode()
        if v.tag == "x":
            return "text", bytes(v.value)
        if v.tag == "t":
            return "text", b"true" if v.value else b"false"
        return "raw", v.tag, encode_table({"k": v})[4 + 3:]
    if v is None:
        return "text", b""
    if isinstance(v, bool):
        return "text", b"true" if v else b"false"
    if isinstance(v, int):
        return "text", str(v).encode()
    if isinstance(v, str):
        return "text", v.encode()
    if isinstance(v, (bytes, bytearray)):
        return "text", bytes(v)
    wire = encode_table({"k": v})[4 + 2:]        # tag, then the value's wire bytes
    return "raw", chr(wire[0]), wire[1:]


def brute_match(args, headers):
    """``args``: a binding's arguments {name: value}; ``headers``: the message's entries
    [(name, value)] in table order (None or []: no headers)."""
    mode = "all"
    if "x-match" in args and text_of(args["x-match"]) == ("text", b"any"):
        mode = "any"
    pairs = [(k, v) for k, v in args.items() if not k.startswith("x-")]
    first = {}
    for n, v in headers or []:
        first.setdefault(n, v)                       # of duplicate names the first counts
    hits = [k in first and (v is None or text_of(first[k]) == text_of(v)) for k, v in pairs]
    if not pairs:
        return True
    return any(hits) if mode == "any" else all(hits)


# ---------------------------------------------------------------- wire
def table_body(entries):
    """Entries [(name, value)] as a field table's body: duplicates and order kept."""
    return b"".join(encode_table({n: v})[4:] for n, v in entries)


def props_bytes(entries=None, ctype=None, cenc=None, table=None, tail=b"", flags=0):
    """Property bytes: flags, content-type, content-encoding, headers.  ``table``: the headers
    property's bytes as given (length included) instead of ``entries``; ``flags`` / ``tail``:
    further flag bits and the bytes of their fields."""
    out = b""
    if ctype is not None:
        flags |= 1 << 15
        out += bytes([len(ctype)]) + ctype
    if cenc is not None:
        flags |= 1 << 14
        out += bytes([len(cenc)]) + cenc
    if table is None and entries is not None:
        body = table_body(entries)
        table = struct.pack(">I", len(body)) + body
    if table is not None:
        flags |= 1 << 13
        out += table
    return struct.pack(">H", flags) + out + tail


def publish_raw(ch, exchange, key, body, props, mandatory=False, immediate=False, fm=131072):
    m = Method("basic.publish", exchange=exchange, routing_key=key, mandatory=mandatory, immediate=immediate)
    out = [encode_frame(1, ch, m.encode_payload()),
           encode_frame(2, ch, struct.pack(">HHQ", 60, 0, len(body)) + props)]
    step = fm - 8
    out += [encode_frame(3, ch, body[i:i + step]) for i in range(0, len(body), step)]
    return b"".join(out)


class HWorld(World):
    """``World`` with argument bindings, edges and publishes with headers.  ``on`` off: the
    planes were built without headers-match, and a headers exchange routes as topic."""

    def __init__(self, dp, on=True, **kw):
        super().__init__(dp, **kw)
        self.on = on
        self.hbinds = defaultdict(list)      # headers exchange -> [(queue, args)]
        self.edges = defaultdict(list)       # source -> [(destination, key bytes, args)]
        self.headers = None

    def by_args(self, x):
        return self.on and self.xtype.get(x) == "headers"

    def hbind(self, q, x, args, key=""):
        if "arguments" in inspect.signature(self.dp.bind).parameters:
            self.dp.bind(VH, q, x, key, dict(args))
        else:
            self.dp.bind(VH, q, x, key)
        if self.by_args(x):
            if (q, args) not in self.hbinds[x]:
                self.hbinds[x].append((q, args))
        else:
            self.binds[x].append((q, key.encode()))

    def hunbind(self, q, x, args, key=""):
        self.dp.unbind(VH, q, x, key, dict(args))
        self.hbinds[x].remove((q, args))

    def edge(self, dst, src, key="", args=None):
        self.dp.bind_exchange(VH, dst, src, key, args)
        self.edges[src].append((dst, key.encode(), args or {}))

    def hrows(self, x):
        """The exchange's rows as the device table holds them: by queue slot, then by the
        canonical arguments -- here only counted and grouped by queue."""
        return sorted((self.slot[q], q) for q, _ in self.hbinds[x])

    def route_flat(self, x, kb, headers):
        t = self.xtype[x]
        if self.by_args(x):
            hit = {q for q, a in self.hbinds[x] if brute_match(a, headers)}
            nxt = {d for d, _, a in self.edges[x] if brute_match(a, headers)}
        elif t == "direct":
            hit = {q for q, k in self.binds[x] if k == kb}
            nxt = {d for d, k, _ in self.edges[x] if k == kb}
        elif t == "fanout":
            hit = {q for q, _ in self.binds[x]}
            nxt = {d for d, _, _ in self.edges[x]}
        else:
            hit = {q for q, k in self.binds[x] if topic_hit(k, kb, self.hw)}
            nxt = {d for d, k, _ in self.edges[x] if topic_hit(k, kb, self.hw)}
        return hit, nxt

    def route(self, x, key):
        if x not in self.xtype:
            return None
        kb = key.encode() if isinstance(key, str) else key
        hit, seen, todo = set(), set(), [x]
        while todo:                           # every exchange the edges lead to, each once
            cur = todo.pop()
            if cur in seen:
                continue
            seen.add(cur)
            h, nxt = self.route_flat(cur, kb, self.headers)
            hit |= h
            todo += sorted(nxt - seen)
        return sorted(hit, key=self.slot.get)

    def hpub(self, conn, x, headers=None, key="", props=None, size=0, ch=1, mandatory=False, immediate=False,
             emit=True, step_delta=0, **layout):
        """A publish with ``headers`` ([(name, value)] or a dict; None: no headers property).
        ``props``: the property bytes as given, ``headers`` then being what they mean.
        ``emit`` off: the bytes are returned, not sent; ``step_delta``: the publish is
        complete that many steps later."""
        if isinstance(headers, dict):
            headers = list(headers.items())
        self.headers = headers
        routed = self.route(x, key)
        self.headers = None
        ret = 0
        if routed is None:
            routed = []
        elif not routed:
            ret = 312 if mandatory else 0
        elif immediate and not any(q in self.cons for q in routed):
            ret, routed = 313, []
        i = len(self.pubs)
        body = body_of(i, size)
        self.pubs.append(Pub(len(self.steps) + step_delta, conn, ch, i, body, routed, ret, False))
        if props is None:
            props = props_bytes(headers, **layout)
        data = publish_raw(ch, x, key, body, props, mandatory, immediate, self.frame_max.get(conn, 131072))
        if emit:
            self.cur[conn] += data
        return data


def refused(fn, *a, **kw):
    """The call is refused with 506 RESOURCE_ERROR."""
    try:
        fn(*a, **kw)
    except ControlError as e:
        assert e.code == 506, e
        return True
    return False


def table_state(dp):
    return sorted((x.name, len(x.hbindings), len(x.hxbindings), sorted(map(repr, x.hbindings + x.hxbindings)))
                  for x in dp.exchanges.values())


# ================================================================ scenarios
def sc_modes(dp, lim):
    """all, any, no x-match, an unknown x-match value, zero pairs in both modes, x- names
    ignored, a void binding value, a header with another value, an absent header, a message
    without a headers property, and one with an empty table."""
    w = HWorld(dp)
    w.open(1)
    binds = {"q_all": {"x-match": "all", "a": "1", "b": "2"}, "q_any": {"x-match": "any", "a": "1", "b": "2"},
             "q_none": {"a": "1", "b": "2"}, "q_unk": {"x-match": "every", "a": "1", "b": "2"},
             "q_zero_all": {"x-match": "all"}, "q_zero_any": {"x-match": "any"}, "q_zero": {},
             "q_x": {"x-match": "all", "x-ignored": "zz", "a": "1"}, "q_void": {"a": None},
             "q_void_any": {"x-match": "any", "a": None, "z": "9"}, "q_int_mode": {"x-match": 5, "a": "1", "b": "2"}}
    with bulk(dp):
        w.exchange("hx", "headers")
        for q, a in binds.items():
            w.queue(q)
            w.hbind(q, "hx", a, key="rk-" + q)        # the binding's key plays no part
    msgs = [{"a": "1", "b": "2"}, {"a": "1"}, {"a": "1", "b": "3"}, {"b": "2"}, {}, None, {"c": "1"}, {"a": "other"},
            {"x-ignored": "no", "a": "1"}, {"a": "1", "b": "2", "x-match": "any"}, {"z": "9"}]
    zero = ["q_zero_all", "q_zero_any", "q_zero"]
    h = lambda m: (setattr(w, "headers", list(m.items()) if m is not None else None), sorted(w.route("hx", "")))[1]
    assert h(msgs[0]) == sorted(binds) and h(msgs[5]) == sorted(zero) == h(msgs[4]) == h(msgs[6])
    assert h(msgs[1]) == sorted(zero + ["q_any", "q_x", "q_void", "q_void_any"])
    assert h(msgs[7]) == sorted(zero + ["q_void", "q_void_any"]) and h(msgs[10]) == sorted(zero + ["q_void_any"])
    w.headers = None
    for rep, key in ((msgs, ""), (msgs[::-1], "some.key")):     # the publish's key plays no part either
        for m in rep:
            w.hpub(1, "hx", m, key=key)
        w.step()
    w.step()
    return w.run(queues=len(binds))


INT_EDGES = [("b", -128), ("b", 127), ("b", 0), ("b", -1), ("B", 255), ("B", 0), ("s", -32768), ("s", 32767), ("u", 65535),
             ("u", 0), ("I", -(1 << 31)), ("I", (1 << 31) - 1), ("I", -7), ("i", (1 << 32) - 1), ("i", 0),
             ("l", -(1 << 63)), ("l", (1 << 63) - 1), ("l", 0), ("l", -1), ("l", 10 ** 18), ("T", (1 << 63) - 1),
             ("T", 1 << 63), ("T", (1 << 64) - 1), ("T", 0)]


def sc_value_types(dp, lim, raw=True):
    """Every integer tag at its extremes against the equal decimal string and a near miss (one
    header name per case, a hit queue and a miss queue); a string message value against an
    integer binding; t against "true" / "false"; V as message value against ""; and the raw
    class f d D A F (``raw``): equal bytes hit, another tag with the same number and other
    bytes miss."""
    w = HWorld(dp)
    w.open(1)
    cases = []          # (name, binding value, near-miss binding value, message value)
    for i, (tag, v) in enumerate(INT_EDGES):
        seen = v - (1 << 64) if tag == "T" and v >= 1 << 63 else v
        cases.append((f"i{i:02d}", str(seen), str(seen + 1) if seen < 0 else str(seen - 1) if seen else "00", Typed(tag, v)))
    cases += [("sb", Typed("I", 5), Typed("I", 6), "5"), ("sl", Typed("l", -40), Typed("l", 40), "-40"),
              ("neg0", "-0", "+0", Typed("I", 0)), ("lead", "05", " 5", Typed("B", 5)),
              ("tt", "true", "false", True), ("tf", "false", "true", False), ("tT", True, False, "true"),
              ("t1", "true", "1", Typed("t", 7)), ("vv", "", " ", None), ("vs", "", "x", ""),
              ("xs", "bytes", "byte", Typed("x", b"bytes"))]
    # ("neg0", "lead": a binding's text is compared as text: "-0" and "05" are not what 0 and 5 render as)
    flip = {"neg0", "lead"}
    with bulk(dp):
        w.exchange("hv", "headers")
        for name, good, bad, _ in cases:
            for kind, val in (("hit", good), ("miss", bad)):
                w.queue(f"{kind}_{name}", consume=kind == "hit" or name in flip)
                w.hbind(f"{kind}_{name}", "hv", {name: val})
        if raw:
            for q, val in (("r_d", 1.5), ("r_f", Typed("f", 1.5)), ("r_D", Decimal("1.50")), ("r_A", [1, "two"]),
                           ("r_F", {"k": 1}), ("r_s", "1.5")):
                w.queue(q)
                w.hbind(q, "hv", {"r": val})
    for name, _, _, mv in cases:
        p = w.hpub(1, "hv", [(name, mv)])
        assert p is not None and w.pubs[-1].queues == ([] if name in flip else [f"hit_{name}"]), (name, w.pubs[-1].queues)
    w.step()
    if raw:
        want = [(1.5, ["r_d"]), (Typed("f", 1.5), ["r_f"]), (1.25, []), (Decimal("1.50"), ["r_D"]), (Decimal("1.5"), []),
                ([1, "two"], ["r_A"]), ([1, "tw0"], []), ({"k": 1}, ["r_F"]), ({"k": 2}, []), ("1.5", ["r_s"]),
                (Typed("I", 1), [])]
        for mv, qs in want:
            w.hpub(1, "hv", [("r", mv)])
            assert w.pubs[-1].queues == qs, (mv, w.pubs[-1].queues)
        w.step()
    w.step()
    return w.run(cases=len(cases))


def filler(n, at=None, entry=None):
    """n entries f000 .. with ``entry`` at index ``at``."""
    ents = [(f"f{i:03d}", "v") for i in range(n)]
    if at is not None:
        ents[at] = entry
    return ents


def sc_entry_chunks(dp, lim, sizes=(1, 63, 64, 65, 130)):
    """Messages of 1, 63, 64, 65 and 130 entries with the deciding entry first, at index 63,
    at 64 and last (a hit, and with another value a miss); a duplicate name whose first
    occurrence lies in one 64 of entries and whose second, with another value, in the next;
    an ``all`` binding whose pairs lie in both."""
    w = HWorld(dp)
    w.open(1)
    with bulk(dp):
        w.exchange("he", "headers")
        for q, a in (("qk", {"key": "yes"}), ("q1", {"dup": "one"}), ("q2", {"dup": "two"}),
                     ("qs", {"x-match": "all", "f005": "v", "f100": "v"}), ("qz", {})):
            w.queue(q)
            w.hbind(q, "he", a)
    placed = 0
    for n in sizes:
        for at in sorted({0, 63, 64, n - 1}):
            if at >= n:
                continue
            for val in ("yes", "no"):
                w.hpub(1, "he", filler(n, at, ("key", val)))
                assert ("qk" in w.pubs[-1].queues) == (val == "yes")
                placed += 1
        w.step()
    big = max(sizes)
    if big > CHUNK + 6:
        dup = filler(big, 10, ("dup", "one"))
        dup[CHUNK + 6] = ("dup", "two")
        w.hpub(1, "he", dup)
        assert w.pubs[-1].queues == ["q1", "qs", "qz"] if big > 100 else True
        dup[10], dup[CHUNK + 6] = dup[CHUNK + 6], dup[10]
        w.hpub(1, "he", dup)
        assert "q2" in w.pubs[-1].queues and "q1" not in w.pubs[-1].queues
        w.hpub(1, "he", filler(big))
        assert ("qs" in w.pubs[-1].queues) == (big > 100)
    w.hpub(1, "he", filler(65))
    assert "qs" not in w.pubs[-1].queues and "qz" in w.pubs[-1].queues
    w.step()
    w.step()
    return w.run(placed=placed)


ROW_SIZES = (63, 64, 65)


def sc_row_chunks(dp, lim):
    """Exchanges of 63, 64, 65 and 200 rows laid out one behind the other in the row table.
    The 200 rows belong to 20 queues of 10 rows each, so queue 6 holds rows 60..69 across the
    first 64-row edge: its only hit in its first row, in its last, at rows 63 and 64; a
    message that hits all 200 rows reaches every queue once.  The smaller exchanges have one
    row per queue: the hit at row 62, 63 and 64, and all of them at once."""
    w = HWorld(dp)
    w.open(1)
    with bulk(dp):
        for n in ROW_SIZES:
            w.exchange(f"r{n}", "headers")
        w.exchange("r200", "headers")
        for i in range(max(ROW_SIZES)):
            w.queue(f"p{i:02d}")
        for i in range(20):
            w.queue(f"g{i:02d}")
        for n in ROW_SIZES:
            for i in range(n):
                w.hbind(f"p{i:02d}", f"r{n}", {"x-match": "any", "n": str(n), "id": f"{i:02d}"})
        for i in range(20):
            for j in range(10):
                w.hbind(f"g{i:02d}", "r200", {"x-match": "any", "every": "yes", "k": f"{i:02d}-{j}"})
    slots = [dp.exchanges[(VH, x)].slot for x in ("r63", "r64", "r65", "r200")]
    assert slots == sorted(slots) and [len(w.hrows(f"r{n}")) for n in ROW_SIZES] == list(ROW_SIZES)
    rows = w.hrows("r200")
    assert len(rows) == 200 and [q for _, q in rows[60:70]] == ["g06"] * 10 and rows[63][1] == rows[64][1] == "g06"
    if not is_golden(dp):
        assert dp.h_used == (sum(ROW_SIZES) + 200, sum(ROW_SIZES) * 2 + 400)
    for n in ROW_SIZES:
        for i in (0, 62, 63, 64):
            if i < n:
                w.hpub(1, f"r{n}", {"id": f"{i:02d}"})
                assert w.pubs[-1].queues == [f"p{i:02d}"]
        w.hpub(1, f"r{n}", {"n": str(n)})
        assert len(w.pubs[-1].queues) == n
        w.hpub(1, f"r{n}", {"n": str(n + 1), "id": "99"})
        assert w.pubs[-1].queues == []
    w.step()
    for k in ("06-0", "06-9", "06-3", "06-4", "00-0", "19-9", "12-5"):
        w.hpub(1, "r200", {"k": k})
        assert w.pubs[-1].queues == ["g" + k[:2]]
    w.hpub(1, "r200", {"every": "yes"})
    assert len(w.pubs[-1].queues) == 20
    w.hpub(1, "r200", {"every": "no", "k": "20-0"})
    assert w.pubs[-1].queues == []
    w.step()
    w.step()
    return w.run(rows=sum(ROW_SIZES) + 200)


PAIRS_ROWS = 6


def pairs_cfg(lim):
    return dict(hb_max=PAIRS_ROWS, hp_max=2 * lim.HB_PAIRS + 3)


def sc_pairs_max(dp, lim):
    """A binding of exactly HB_PAIRS pairs deciding on the last one; HB_PAIRS + 1 pairs refused
    with 506 and nothing changed; the pair pool filled to its last pair and one past it; the
    row table filled to its last row and one past it; what was bound before still routes."""
    N = lim.HB_PAIRS
    assert (dp.hb_max, dp.hp_max) == (PAIRS_ROWS, 2 * N + 3)
    w = HWorld(dp)
    w.open(1)
    w.exchange("hp", "headers")
    w.exchange("hq", "headers")
    for q in ("full", "a", "b", "c", "d", "e", "f"):
        w.queue(q)
    full = {f"p{i:02d}": str(i) for i in range(N)}
    w.hbind("full", "hp", dict(full, **{"x-match": "all"}))                 # pool: N
    before = table_state(dp)
    assert refused(dp.bind, VH, "a", "hp", "", dict(full, extra="1")) and table_state(dp) == before
    assert refused(dp.bind_exchange, VH, "hq", "hp", "", dict(full, extra="1")) and table_state(dp) == before
    w.hbind("a", "hp", {f"p{i:02d}": str(i) for i in range(N)} | {"x-match": "any"})      # pool: 2 N
    w.hbind("b", "hp", {"u": "1", "v": "2"})                                # pool: 2 N + 2
    before = table_state(dp)
    assert refused(dp.bind, VH, "c", "hp", "", {"u": "1", "v": "2"}) and table_state(dp) == before   # one past the pool
    w.hbind("c", "hp", {"u": "1"})                                          # pool: 2 N + 3, its last pair
    before = table_state(dp)
    assert refused(dp.bind, VH, "d", "hq", "", {"w": "1"}) and table_state(dp) == before
    w.hbind("d", "hq", {})                                                  # rows: 5
    w.edge("hq", "hp", args={})                                             # rows: 6, the last
    before = table_state(dp)
    assert refused(dp.bind, VH, "e", "hq", "", {}) and table_state(dp) == before
    assert refused(dp.bind_exchange, VH, "hp", "hq", "", {}) and table_state(dp) == before
    w.hbind("d", "hq", {})                                                  # a duplicate: a no-op, not a refusal
    assert table_state(dp) == before
    last = f"p{N - 1:02d}"
    good = [(k, v) for k, v in full.items()]
    w.hpub(1, "hp", good)
    assert w.pubs[-1].queues == ["full", "a", "d"]
    w.hpub(1, "hp", good[:-1] + [(last, "wrong")])
    assert w.pubs[-1].queues == ["a", "d"]
    w.hpub(1, "hp", [(last, str(N - 1))])
    assert w.pubs[-1].queues == ["a", "d"]
    w.hpub(1, "hp", {"u": "1"})
    assert w.pubs[-1].queues == ["c", "d"]
    w.hpub(1, "hq", {"u": "1"})
    assert w.pubs[-1].queues == ["d"]
    w.step()
    w.step()
    return w.run(pairs=N)


NAME_PAIR = ("pypkvrmqpa", "wdnbhcxbkd")       # two strings with one 32-bit FNV-1a hash each
VALUE_PAIR = ("jwimvqwecr", "taoqorwdtt")


def sc_collisions(dp, lim):
    """Names and values whose 32-bit FNV-1a hashes are equal: the hash is a prefilter, the
    bytes decide.  A binding on one must not match a message carrying the other."""
    for a, b in (NAME_PAIR, VALUE_PAIR):
        assert a != b and len(a) == len(b) and fnv32(a.encode()) == fnv32(b.encode())
    w = HWorld(dp)
    w.open(1)
    with bulk(dp):
        w.exchange("hc", "headers")
        for q, a in (("n0", {NAME_PAIR[0]: "v"}), ("n1", {NAME_PAIR[1]: "v"}), ("np", {NAME_PAIR[0]: None}),
                     ("v0", {"h": VALUE_PAIR[0]}), ("v1", {"h": VALUE_PAIR[1]}),
                     ("both", {NAME_PAIR[0]: VALUE_PAIR[0]})):
            w.queue(q)
            w.hbind(q, "hc", a)
    for m, qs in (({NAME_PAIR[0]: "v"}, ["n0", "np"]), ({NAME_PAIR[1]: "v"}, ["n1"]), ({"h": VALUE_PAIR[0]}, ["v0"]),
                  ({"h": VALUE_PAIR[1]}, ["v1"]), ({NAME_PAIR[0]: VALUE_PAIR[0]}, ["np", "both"]),
                  ({NAME_PAIR[0]: VALUE_PAIR[1]}, ["np"]), ({NAME_PAIR[1]: VALUE_PAIR[0]}, []),
                  ([(NAME_PAIR[1], "v"), (NAME_PAIR[0], "v")], ["n0", "n1", "np"])):
        w.hpub(1, "hc", m)
        assert w.pubs[-1].queues == qs, (m, w.pubs[-1].queues)
    w.step()
    w.step()
    return w.run()


def sc_layout(dp, lim):
    """Headers behind a content-type and a content-encoding of 0, 1 and 255 bytes and behind
    neither; names of 1 and 255 bytes; string values of 0, 1, 255, 256 and 4096 bytes; further
    properties behind the headers; a publish that arrives split over two steps."""
    w = HWorld(dp)
    w.open(1)
    long_name = "N" * 255
    vals = {n: "s" * n for n in (0, 1, 255, 256, 4096)}
    with bulk(dp):
        w.exchange("hl", "headers")
        w.queue("k")
        w.hbind("k", "hl", {"a": "1"})
        w.queue("n1")
        w.hbind("n1", "hl", {"z": "1"})
        w.queue("n255")
        w.hbind("n255", "hl", {long_name: "1"})
        for n, v in vals.items():
            w.queue(f"v{n}")
            w.hbind(f"v{n}", "hl", {"val": v})
    for ct in (None, b"", b"c", b"c" * 255):
        for ce in (None, b"", b"e", b"e" * 255):
            w.hpub(1, "hl", {"a": "1"}, ctype=ct, cenc=ce)
            assert w.pubs[-1].queues == ["k"]
    w.step()
    w.hpub(1, "hl", {"z": "1"})
    w.hpub(1, "hl", {long_name: "1"})
    w.hpub(1, "hl", {long_name[:-1]: "1"})
    assert [p.queues for p in w.pubs[-3:]] == [["n1"], ["n255"], []]
    for n, v in vals.items():
        w.hpub(1, "hl", [("pad", "x" * 300), ("val", v)])
        assert w.pubs[-1].queues == [f"v{n}"]
    w.hpub(1, "hl", {"val": "s" * 4095})
    assert w.pubs[-1].queues == []
    # delivery-mode, priority, message-id and timestamp behind the headers
    w.hpub(1, "hl", {"a": "1"}, flags=(1 << 12) | (1 << 11) | (1 << 7) | (1 << 6),
           tail=b"\x01\x05" + b"\x03mid" + struct.pack(">Q", 1_700_000_000))
    assert w.pubs[-1].queues == ["k"]
    w.step()
    data = w.hpub(1, "hl", [("pad", "y" * 700), ("a", "1")], size=900, emit=False, step_delta=1)
    assert w.pubs[-1].queues == ["k"]
    cut = len(data) - 1200          # inside the header frame's table
    w.send(1, data[:cut])
    w.step()
    w.send(1, data[cut:])
    w.step()
    w.step()
    return w.run()


def sc_malformed(dp, lim):
    """Messages whose headers cannot be read have no headers: only the bindings without pairs
    match.  The table's length running past the property list; an unknown tag in the middle;
    an entry running past the table; a property list cut short behind a sound table."""
    w = HWorld(dp)
    w.open(1)
    with bulk(dp):
        w.exchange("hm", "headers")
        for q, a in (("zero", {}), ("zero_any", {"x-match": "any"}), ("one", {"a": "1"}),
                     ("any", {"x-match": "any", "a": "1", "b": "2"}), ("void", {"a": None})):
            w.queue(q)
            w.hbind(q, "hm", a)
    good = table_body([("a", "1"), ("b", "2")])
    sound = props_bytes(table=struct.pack(">I", len(good)) + good)
    bad = {
        "sound": (sound, [("a", "1"), ("b", "2")]),
        "table_past_list": (props_bytes(table=struct.pack(">I", len(good) + 1) + good), None),
        "unknown_tag": (props_bytes(table=struct.pack(">I", len(good) + 4) + table_body([("a", "1")]) + b"\x01uU1"
                                    + table_body([("b", "2")])), None),
        "entry_past_table": (props_bytes(table=struct.pack(">I", len(good) - 1) + good[:-1]), None),
        "name_past_table": (props_bytes(table=struct.pack(">I", len(good) + 2) + good + b"\x09n"), None),
        "list_cut": (props_bytes(table=struct.pack(">I", len(good)) + good, flags=1 << 7, tail=b"\x05mi"), None),
        "flags_cut": (b"\x20\x01", None),
    }
    for name, (props, means) in bad.items():
        w.hpub(1, "hm", means, props=props)
        assert w.pubs[-1].queues == (["zero", "zero_any", "one", "any", "void"] if means else ["zero", "zero_any"]), name
    w.step()
    w.step()
    return w.run(shapes=len(bad))


def sc_outcomes(dp, lim):
    """The headers exchange in the outcomes a publish can have: mandatory with no match (312,
    nothing stored), immediate with and without a consumer, a confirm channel, PUB_QC,
    PUB_QC + 1 and 130 matching queues (pass 1 routes again), and groups of 16 publishes that
    mix headers, topic, direct and fanout exchanges."""
    Q = lim.PUB_QC
    w = HWorld(dp)
    w.open(1, confirm=True)
    w.open(3)
    with bulk(dp):
        w.exchange("ho", "headers")
        w.exchange("tx", "topic")
        w.exchange("dx", "direct")
        w.exchange("fx", "fanout")
        for i in range(130):
            w.queue(f"q{i:03d}")
            w.hbind(f"q{i:03d}", "ho", {"x-match": "any", "all": "130", "q": str(i)})
            if i < Q:
                w.hbind(f"q{i:03d}", "ho", {"n": str(Q)})
            if 40 <= i < 41 + Q:
                w.hbind(f"q{i:03d}", "ho", {"n": str(Q + 1)})
        w.queue("lonely", consume=False)
        w.hbind("lonely", "ho", {"who": "lonely"})
        w.bind("q000", "tx", "t.*")
        w.bind("q001", "dx", "k")
        w.bind("q002", "fx", "")
        w.bind("q003", "fx", "")
    kinds = [lambda c: w.hpub(c, "ho", {"n": str(Q)}), lambda c: w.hpub(c, "ho", {"n": str(Q + 1)}),
             lambda c: w.hpub(c, "ho", {"all": "130"}), lambda c: w.hpub(c, "ho", {"none": "1"}, mandatory=True),
             lambda c: w.hpub(c, "ho", {"none": "1"}), lambda c: w.hpub(c, "ho", {"who": "lonely"}, immediate=True),
             lambda c: w.hpub(c, "ho", {"q": "77"}, immediate=True), lambda c: w.pub(c, "tx", "t.1"),
             lambda c: w.pub(c, "dx", "k"), lambda c: w.pub(c, "fx", "any"), lambda c: w.hpub(c, "ho", {"q": "5"}),
             lambda c: w.hpub(c, "ho", None, mandatory=True), lambda c: w.pub(c, "dx", "lost", mandatory=True)]
    at = 0
    for n, conn in ((16, 1), (17, 1), (5, 3), (33, 1)):
        for _ in range(n):
            kinds[at % len(kinds)](conn)
            at += 1
        w.step()
    w.step()
    sizes = {len(p.queues) for p in w.pubs}
    assert {Q, Q + 1, 130, 0, 1, 2} <= sizes and {p.ret for p in w.pubs} == {0, 312, 313}
    return w.run()


def sc_walk(dp, lim):
    """Exchange-to-exchange edges through headers exchanges: topic -> headers -> fanout; a
    headers source whose edges have arguments, one matching and one not; a cycle through a
    headers exchange; a queue reached both directly and over an edge (one copy)."""
    w = HWorld(dp)
    w.open(1)
    with bulk(dp):
        for x, t in (("t0", "topic"), ("h1", "headers"), ("f2", "fanout"), ("h3", "headers"), ("d4", "direct"),
                     ("h5", "headers"), ("f6", "fanout")):
            w.exchange(x, t)
        for q in ("qt", "qh", "qf", "qa", "qb", "qc", "both", "far"):
            w.queue(q)
        w.bind("qt", "t0", "go.*")
        w.edge("h1", "t0", "go.#")
        w.hbind("qh", "h1", {"kind": "a"})
        w.edge("f2", "h1", args={"x-match": "any", "kind": "a", "fan": "yes"})
        w.bind("qf", "f2", "")
        w.bind("both", "f2", "")
        w.hbind("both", "h1", {"kind": "a"})
        # a headers source with two edges, and a cycle h3 -> d4 -> h5 -> h3
        w.hbind("qa", "h3", {"kind": "b"})
        w.edge("d4", "h3", args={"kind": "b"})
        w.edge("f6", "h3", args={"kind": "never"})
        w.bind("qb", "d4", "dk")
        w.edge("h5", "d4", "dk")
        w.hbind("qc", "h5", {"x-match": "any", "kind": "b", "other": "1"})
        w.edge("h3", "h5", args={})
        w.bind("far", "f6", "")
    for x, key, m, qs in (("t0", "go.1", {"kind": "a"}, ["qt", "qh", "qf", "both"]), ("t0", "go.1", {"kind": "z"}, ["qt"]),
                          ("t0", "go.1", {"fan": "yes"}, ["qt", "qf", "both"]), ("t0", "stay", {"kind": "a"}, []),
                          ("h1", "", {"kind": "a"}, ["qh", "qf", "both"]), ("h3", "dk", {"kind": "b"}, ["qa", "qb", "qc"]),
                          ("h3", "other", {"kind": "b"}, ["qa"]), ("h5", "dk", {"other": "1"}, ["qc"]),
                          ("h5", "dk", {"kind": "b"}, ["qa", "qb", "qc"]), ("d4", "dk", None, ["qb"]),
                          ("h3", "dk", {"kind": "never"}, ["far"])):
        w.hpub(1, x, m, key=key)
        assert w.pubs[-1].queues == qs, (x, key, m, w.pubs[-1].queues)
    w.step()
    w.step()
    return w.run()


def sc_off_is_today(dp, lim):
    """With the option off a headers exchange routes as topic on the two keys, and binding
    arguments and message headers play no part."""
    w = HWorld(dp, on=False)
    w.open(1)
    with bulk(dp):
        w.exchange("hx", "headers")
        for q, key, a in (("q_a", "a.*", {"x-match": "all", "h": "1"}), ("q_b", "#", {"h": "2"}), ("q_c", "", {})):
            w.queue(q)
            w.hbind(q, "hx", a, key=key)
    for key, m, qs in (("a.b", {"h": "2"}, ["q_a", "q_b"]), ("", {"h": "1"}, ["q_b", "q_c"]), ("c", None, ["q_b"])):
        w.hpub(1, "hx", m, key=key)
        assert w.pubs[-1].queues == qs
    w.step()
    w.step()
    assert all(not x.hbindings for x in dp.exchanges.values() if hasattr(x, "hbindings"))
    return w.run()


BIG = dict(q_max=256, hb_max=512, hp_max=1024)
SCENARIOS = {
    "modes": Scenario(sc_modes, HCFG, 0, True, True),
    "value_types": Scenario(sc_value_types, dict(HCFG, q_max=128, hb_max=128), 0, True, True),
    "entry_chunks": Scenario(sc_entry_chunks, HCFG, 0, True, True),
    "row_chunks": Scenario(sc_row_chunks, dict(BIG, q_max=128), 0, True, True),
    "pairs_max": Scenario(sc_pairs_max, pairs_cfg, 0, True, True),
    "collisions": Scenario(sc_collisions, HCFG, 0, True, True),
    "layout": Scenario(sc_layout, HCFG, 0, True, True),
    "malformed": Scenario(sc_malformed, HCFG, 0, True, True),
    "outcomes": Scenario(sc_outcomes, BIG, 0, True, False),
    "walk": Scenario(sc_walk, HCFG, 0, True, True),
}
OFF = Scenario(sc_off_is_today, {}, 0, True, True)


def cfg_of(sc, base, lim):
    return dict(base, **(sc.cfg(lim) if callable(sc.cfg) else sc.cfg))


# ================================================================ sharded
# (world, exchange) -> queues (name, owning rank, arguments); the message {"k": <exchange>}
# matches the queues marked in SHARD_HITS: one remote queue (it travels with the record:
# MF_ONEQ), one remote + one local, two remote on one rank (the owner matches again, from the
# record's own property bytes, and must leave the third queue there out), two remote on two
# ranks
SHARD_TOPO = {
    "one_remote": [("a_hit", 1, {"k": "one_remote"}), ("a_no", 1, {"k": "zz"})],
    "remote_local": [("b_loc", 0, {"k": "remote_local"}), ("b_rem", 1, {"k": "remote_local"}), ("b_no", 0, {"k": "zz"})],
    "two_on_one": [("c_1", 1, {"k": "two_on_one"}), ("c_2", 1, {"x-match": "any", "k": "two_on_one", "z": "1"}),
                   ("c_no", 1, {"k": "other"}), ("c_void", 1, {"only": None})],
    "two_ranks": [("d_1", 1, {"k": "two_ranks"}), ("d_2", 2, {"k": "two_ranks"}), ("d_no", 2, {"k": "nope"})],
}
SHARD_STEPS = 4
PUB_CONN, CONS_CONN = 1, 10


def sharded_cluster(cfg, world, lag=0, gpu=False, graph=True):
    from chanamq_amd.parallel.cluster import LocalCluster
    from xchg_scenarios import golden_kw
    if gpu:
        import torch

        from chanamq_amd.engine.dataplane import GpuDataPlane
        torch.cuda.set_device(0)
        return LocalCluster(lambda **k: GpuDataPlane(graph=graph, exchange_lag=lag, headers_match=True,
                                                     **dict(cfg, **HCFG), **k), world)
    from chanamq_amd.engine.golden import GoldenDataPlane
    return LocalCluster(lambda **k: GoldenDataPlane(exchange_lag=lag, headers_match=True, **golden_kw(cfg), **k), world)


def shard_cases(world):
    return [x for x in sorted(SHARD_TOPO) if all(r < world for _, r, _ in SHARD_TOPO[x])]


def sharded_run(cl, now=1_800_000_000_000):
    """Declare SHARD_TOPO on every rank of the cluster, publish from rank 0 and step
    SHARD_STEPS times.  -> (per rank and step {conn: egress bytes}, {queue: [bodies]} expected)."""
    world = cl.world
    xs = shard_cases(world)
    for x in xs:
        for q, r, _ in SHARD_TOPO[x]:
            cl.shard_map.place(VH, q, r)
    for p in cl.planes:
        for x in xs:
            p.declare_exchange(VH, x, "headers")
            for q, r, a in SHARD_TOPO[x]:
                p.declare_queue(VH, q, capacity=64)
                p.bind(VH, q, x, "", a)
        p.open_connection(CONS_CONN, VH)
        p.open_channel(CONS_CONN, 1)
        for x in xs:
            for q, r, _ in SHARD_TOPO[x]:
                if r == p.rank:
                    p.consume(CONS_CONN, 1, VH, q, q, no_ack=True)
    cl[0].open_connection(PUB_CONN, VH)
    cl[0].open_channel(PUB_CONN, 1)
    data, want, i = b"", defaultdict(list), 0
    for rep in range(2):
        for x in xs:
            for hdrs in ([("k", x)], [("k", "yy")], None, [("z", "1"), ("only", Typed("I", 0))], [("k", x), ("k", "zz")]):
                body = body_of(i)
                i += 1
                for q, _, a in SHARD_TOPO[x]:
                    if brute_match(a, hdrs):
                        want[q].append(body)
                data += publish_raw(1, x, "any.key", body, props_bytes(hdrs))
    outs = [[] for _ in range(world)]
    for k in range(SHARD_STEPS):
        res = cl.step([{PUB_CONN: data} if k == 0 else {}] + [{} for _ in range(world - 1)], now_ms=now + k)
        for r, o in enumerate(res):
            outs[r].append(dict(o["egress"] if isinstance(o, dict) else o.egress))
    assert {q for q, v in want.items() if v} >= {"a_hit", "b_loc", "b_rem", "c_1", "c_2", "c_void"}
    assert not want.get("a_no") and not want.get("c_no") and not want.get("b_no")
    return outs, dict(want)


def sharded_got(outs):
    """{queue: [bodies]} delivered, by consumer tag, over all ranks and steps."""
    from route_scenarios import observe
    got = defaultdict(list)
    for per_rank in outs:
        for s in observe([dict(egress={c: e for c, e in o.items() if c == CONS_CONN}) for o in per_rank]):
            assert s.kind == "deliver"
            got[s.ctag].append(s.body)
    return dict(got)
