"""Golden routing matchers (direct / fanout / topic / headers).

Reference: chana-mq-server/.../engine/QueueMatcher.scala
  * trait QueueMatcher {subscribe, unsubscribe, lookup}      :11-27
  * DirectMatcher: exact key -> subscribers                   :29-48
  * FanoutMatcher: every subscriber, key ignored              :50-66
  * TrieMatcher: words split on regex "\\." (Java split drops trailing
    empty strings), '*' matches exactly one word             :68-601
    The reference treats '#' literally (getBranches :261-263); SURVEY §7.4
    recommends standard AMQP '#' (zero or more words).  ``hash_wildcard``
    selects: True (default, AMQP 0-9-1 semantics) or False (reference parity).

These are the host golden models the HIP route kernels (K6) are tested against.
The GPU path stores the same word tokenisation (``split_words``).

Headers exchanges (``chana.mq.gpu.headers-match``): ``headers_match`` below is the one
statement of the rule; the golden model, ``ControlState`` and the device branch of
``route_one`` (csrc/kernels/dp_headers.h) all answer to it.  CHANGES.md "Headers exchanges".
"""

import struct


def split_words(key: str):
    """Java ``String.split("\\\\.")`` semantics (trailing empty strings dropped)."""
    if key == "":
        return [""]
    parts = key.split(".")
    while parts and parts[-1] == "":
        parts.pop()
    return parts


def topic_match(pattern: str, key: str, hash_wildcard: bool = True) -> bool:
    pw = split_words(pattern)
    kw = split_words(key)
    return words_match(pw, kw, hash_wildcard)


def words_match(pw, kw, hash_wildcard=True) -> bool:
    # dynamic programming over (pattern word, key word); O(|p|*|k|)
    np_, nk = len(pw), len(kw)
    reach = [False] * (nk + 1)
    reach[0] = True
    for i in range(np_):
        w = pw[i]
        nxt = [False] * (nk + 1)
        if hash_wildcard and w == "#":
            acc = False
            for j in range(nk + 1):
                acc = acc or reach[j]
                nxt[j] = acc
        else:
            for j in range(nk):
                if reach[j] and (w == "*" or w == kw[j]):
                    nxt[j + 1] = True
        reach = nxt
    return reach[nk]


class QueueMatcher:
    def subscribe(self, key, subscriber):
        raise NotImplementedError

    def unsubscribe(self, key, subscriber):
        raise NotImplementedError

    def lookup(self, key):
        raise NotImplementedError


class DirectMatcher(QueueMatcher):
    def __init__(self):
        self.table = {}

    def subscribe(self, key, sub):
        self.table.setdefault(key, set()).add(sub)

    def unsubscribe(self, key, sub):
        s = self.table.get(key)
        if s is not None:
            s.discard(sub)
            if not s:
                del self.table[key]

    def unsubscribe_all(self, sub):
        for k in list(self.table):
            self.unsubscribe(k, sub)

    def lookup(self, key):
        return set(self.table.get(key, ()))

    def bindings(self):
        return [(k, s) for k, subs in self.table.items() for s in subs]


class FanoutMatcher(QueueMatcher):
    def __init__(self):
        self.subs = {}  # sub -> set(keys)

    def subscribe(self, key, sub):
        self.subs.setdefault(sub, set()).add(key)

    def unsubscribe(self, key, sub):
        ks = self.subs.get(sub)
        if ks is not None:
            ks.discard(key)
            if not ks:
                del self.subs[sub]

    def unsubscribe_all(self, sub):
        self.subs.pop(sub, None)

    def lookup(self, key):
        return set(self.subs)

    def bindings(self):
        return [(k, s) for s, ks in self.subs.items() for k in ks]


class TopicMatcher(QueueMatcher):
    """Pattern list + DP match.  (The reference's CAS trie exists only to be
    lock-free inside one actor — SURVEY §5.2 — so a flat list is the honest
    golden model; the device kernel is the fast path.)"""

    def __init__(self, hash_wildcard=True):
        self.patterns = {}  # pattern -> set(subs)
        self.hash_wildcard = hash_wildcard

    def subscribe(self, key, sub):
        self.patterns.setdefault(key, set()).add(sub)

    def unsubscribe(self, key, sub):
        s = self.patterns.get(key)
        if s is not None:
            s.discard(sub)
            if not s:
                del self.patterns[key]

    def unsubscribe_all(self, sub):
        for k in list(self.patterns):
            self.unsubscribe(k, sub)

    def lookup(self, key):
        kw = split_words(key)
        out = set()
        for p, subs in self.patterns.items():
            if words_match(split_words(p), kw, self.hash_wildcard):
                out |= subs
        return out

    def bindings(self):
        return [(k, s) for k, subs in self.patterns.items() for s in subs]


def make_matcher(ex_type: str, hash_wildcard=True) -> QueueMatcher:
    """direct/fanout as named; topic, headers and any other type route via topic
    (ExchangeEntity.scala:149-154,211-216)."""
    if ex_type == "direct":
        return DirectMatcher()
    if ex_type == "fanout":
        return FanoutMatcher()
    return TopicMatcher(hash_wildcard)


# ---------------------------------------------------------------------------- headers
# The rule is the native host broker's (csrc/core/broker.cpp headers_match / table_str):
#   * x-match "any", or anything else (absent included) = all;
#   * binding arguments whose name starts with "x-" are not pairs;
#   * a pair hits when the message has a header of that name and the binding's value is
#     void ('V': presence only) or both canonical values are equal;
#   * all: every pair hits; any: at least one does; zero pairs match everything;
#   * neither routing key takes part; the first of duplicate names in a message counts.
# Canonical value = (class, bytes).  TEXT: 'S' / 'x' their bytes, 't' true / false, 'V'
# empty, the integer tags their decimal text (width and signedness as csrc/core/codec.cpp
# reads them: 'T' is signed there).  RAW ('f' 'd' 'D' 'A' 'F'): the tag byte and the raw
# wire bytes -- equal only to the same tag with the same bytes (the host renders floats;
# the device does not: CHANGES.md).
FNV32_BASIS, FNV32_PRIME = 0x811C9DC5, 0x01000193
TEXT, RAW = 0, 1
INT_TAGS = {"b": (1, True), "B": (1, False), "s": (2, True), "u": (2, False), "I": (4, True), "i": (4, False),
            "l": (8, True), "T": (8, True)}
FIXED_TAGS = {"t": 1, "V": 0, "f": 4, "d": 8, "D": 5}
FIXED_TAGS.update({t: n for t, (n, _) in INT_TAGS.items()})
SIZED_TAGS = "SxAF"          # a 4-byte length, then that many bytes
RAW_TAGS = "fdDAF"


def fnv1a32(b) -> int:
    h = FNV32_BASIS
    for c in bytes(b):
        h = ((h ^ c) * FNV32_PRIME) & 0xFFFFFFFF
    return h


def canon_wire(tag: str, raw: bytes):
    """(class, bytes) of a field value given as its tag and its wire bytes (for the sized
    tags: the 4-byte length included)."""
    if tag in "Sx":
        return TEXT, bytes(raw[4:])
    if tag == "t":
        return TEXT, b"true" if raw[0] else b"false"
    if tag == "V":
        return TEXT, b""
    if tag in INT_TAGS:
        return TEXT, b"%d" % int.from_bytes(raw, "big", signed=INT_TAGS[tag][1])
    if tag in RAW_TAGS:
        return RAW, tag.encode() + bytes(raw)
    raise ValueError(f"unknown field tag {tag!r}")


def canon_value(v):
    """(tag, (class, bytes)) of a decoded field value (protocol/codec.py's Python forms)."""
    from ..protocol.codec import _encode_value
    w = bytearray()
    _encode_value(w, v)
    tag = chr(w[0])
    return tag, canon_wire(tag, bytes(w[1:]))


def _name_bytes(k):
    return k.encode("utf-8", "surrogateescape") if isinstance(k, str) else bytes(k)


def canon_args(arguments):
    """Binding arguments -> (any, pairs): ``any`` the x-match mode, ``pairs`` a sorted tuple
    of (name bytes, presence only, class, value bytes).  Two bindings are the same binding
    iff these are equal.  A value already in this form is returned as it is."""
    if isinstance(arguments, tuple) and len(arguments) == 2 and isinstance(arguments[0], bool):
        return arguments[0], tuple(tuple(p) for p in arguments[1])
    any_, pairs = False, []
    for k, v in (arguments or {}).items():
        name = _name_bytes(k)
        tag, (cls, val) = canon_value(v)
        if name == b"x-match":
            any_ = (cls, val) == (TEXT, b"any")
        if name.startswith(b"x-"):
            continue
        pairs.append((name, tag == "V", cls, b"" if tag == "V" else val))
    return any_, tuple(sorted(pairs))


def table_entries(tb):
    """Entries [(name bytes, tag, wire bytes)] of a field table's body, None when it is
    malformed: an unknown tag, or an entry running past the table.  Nested tables and arrays
    are taken whole by their length, not looked into."""
    out, pos, end = [], 0, len(tb)
    while pos < end:
        nl = tb[pos]
        if pos + 1 + nl + 1 > end:
            return None
        name = bytes(tb[pos + 1:pos + 1 + nl])
        tag = chr(tb[pos + 1 + nl])
        pos += 2 + nl
        if tag in FIXED_TAGS:
            n = FIXED_TAGS[tag]
        elif tag in SIZED_TAGS:
            if pos + 4 > end:
                return None
            n = 4 + struct.unpack_from(">I", tb, pos)[0]
        else:
            return None
        if pos + n > end:
            return None
        out.append((name, tag, bytes(tb[pos:pos + n])))
        pos += n
    return out


# Basic properties in flag-bit order 15 .. 2: s = shortstr, T = table, o = octet, q = 8 bytes
_PROP_KINDS = "ssToossssqssss"


def props_table(props):
    """The body of the headers table in a publish's property bytes (flags chain, then the
    values), b"" when there is none.  None when the list is cut short anywhere -- inside the
    flags, or inside any field, the ones behind the headers included: such a message has no
    properties (k_decode reads it so), and so no headers."""
    props = bytes(props)
    pos, end, first = 0, len(props), None
    while True:
        if pos + 2 > end:
            return None
        fw = (props[pos] << 8) | props[pos + 1]
        pos += 2
        if first is None:
            first = fw
        if not fw & 1:
            break
    table = b""
    for i, kind in enumerate(_PROP_KINDS):
        if not first & (1 << (15 - i)):
            continue
        if kind == "s":
            if pos + 1 > end:
                return None
            n = 1 + props[pos]
        elif kind == "T":
            if pos + 4 > end:
                return None
            n = 4 + struct.unpack_from(">I", props, pos)[0]
            table = props[pos + 4:pos + n]
        else:
            n = 1 if kind == "o" else 8
        pos += n
        if pos > end:
            return None
    return table


def props_headers(props):
    """{name bytes: (class, value bytes)} of a publish's property bytes: the first of
    duplicate names counts; {} without a headers table, with a cut property list or a
    malformed table."""
    tb = props_table(props)
    ents = table_entries(tb) if tb else None
    out = {}
    for name, tag, raw in ents or ():
        out.setdefault(name, canon_wire(tag, raw))
    return out


def headers_match(binding_args, message_headers) -> bool:
    """``binding_args``: a binding's arguments (a dict of decoded values, or ``canon_args``
    of one); ``message_headers``: the publish's property bytes, or ``props_headers`` of
    them."""
    any_, pairs = canon_args(binding_args)
    hdrs = message_headers if isinstance(message_headers, dict) else props_headers(message_headers)
    hits = 0
    for name, void, cls, val in pairs:
        got = hdrs.get(name)
        if got is not None and (void or got == (cls, val)):
            hits += 1
    if any_:
        return not pairs or hits > 0
    return hits == len(pairs)


# ---- canonical arguments in other clothes: JSON for the replicated control log, a
# string map for the store's bind rows (one row per exchange, queue and key: it holds every
# binding of that triple).  Both give back the same canonical arguments, void and raw values
# included.
def args_json(cargs):
    any_, pairs = canon_args(cargs)
    return {"any": any_, "pairs": [[n.hex(), bool(v), int(c), b.hex()] for n, v, c, b in pairs]}


def args_unjson(j):
    if not isinstance(j, dict) or set(j) != {"any", "pairs"} or not isinstance(j["pairs"], list):
        return j            # (not this form: a plain arguments dict, or None)
    return bool(j["any"]), tuple(sorted((bytes.fromhex(n), bool(v), int(c), bytes.fromhex(b)) for n, v, c, b in j["pairs"]))


def args_to_map(bindings):
    """[canonical arguments] of the bindings of one (exchange, queue, key) -> {str: str}."""
    out = {"n": str(len(bindings))}
    for i, (any_, pairs) in enumerate(bindings):
        out[f"{i}/m"] = "any" if any_ else "all"
        for name, void, cls, val in pairs:
            out[f"{i}/p/{name.hex()}"] = "V" if void else ("R" if cls == RAW else "T") + val.hex()
    return out


def args_from_map(m):
    """The inverse of ``args_to_map``; an empty map (a row written with the option off, or by
    another front end) is one binding without arguments."""
    if "n" not in m:
        return [(False, ())]
    out = []
    for i in range(int(m["n"])):
        pairs = []
        for k, v in m.items():
            if k.startswith(f"{i}/p/"):
                name = bytes.fromhex(k[len(f"{i}/p/"):])
                pairs.append((name, v == "V", RAW if v[:1] == "R" else TEXT, b"" if v == "V" else bytes.fromhex(v[1:])))
        out.append((m.get(f"{i}/m") == "any", tuple(sorted(pairs))))
    return out
