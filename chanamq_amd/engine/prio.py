"""Priority queues (chana.mq.gpu.priority-queues): the golden model's form of
csrc/kernels/prio_plan.h -- the priority of a property list and the lane it selects -- and the
patch of a rendered Basic.GetOk's message-count that both data planes use between steps.

The walk is written out here, not taken from the codec: it is the specification the device's walk
is held to byte for byte (tests/test_prio_plan.py holds both to the codec as well)."""

import struct

PRIO_MAX = 15


def prio_of_props(props):
    """The ``priority`` octet of a Basic property list (flags + values); 0 when absent.  The whole
    list is walked, as k_decode walks it: a list cut short inside any field has no properties at
    all, so its priority is 0 whatever stood ahead of the cut."""
    p = bytes(props)
    n = len(p)
    q = 0
    fl = None
    while True:
        if q + 2 > n:
            return 0   # cut short inside the flags
        fw = (p[q] << 8) | p[q + 1]
        q += 2
        if fl is None:
            fl = fw
        if not fw & 1:
            break
    prio = 0
    for bit in range(15, 1, -1):
        if not fl & (1 << bit):
            continue
        if bit == 13:   # headers table
            if q + 4 > n:
                return 0
            tl = struct.unpack_from(">I", p, q)[0]
            if tl > n - q - 4:
                return 0
            q += 4 + tl
        elif bit in (12, 11):   # delivery-mode, priority
            if q + 1 > n:
                return 0
            if bit == 11:
                prio = p[q]
            q += 1
        elif bit == 6:   # timestamp
            if q + 8 > n:
                return 0
            q += 8
        else:   # short strings
            if q + 1 > n or p[q] > n - q - 1:
                return 0
            q += 1 + p[q]
    return prio


def lane_of(prio, max_priority):
    """Lane slot offset (0 = the base slot, priority P) of a message of priority ``prio``."""
    return max_priority - min(prio, max_priority)


def split_piece(counts, off, cnt):
    """The parts ``(lane, pos, cnt)`` of the piece [off, off + cnt) of V, the concatenation of lanes
    holding ``counts`` ready entries, in lane order (prio_split in prio_plan.h)."""
    out, base = [], 0
    for lane, n in enumerate(counts):
        if cnt <= 0:
            break
        end = base + n
        if off < end:
            take = min(end - off, cnt)
            out.append((lane, off - base, take))
            off += take
            cnt -= take
        base = end
    return out


def patch_getok_count(frames, count):
    """A rendered Basic.GetOk (method frame first) with its message-count replaced by ``count``."""
    b = bytearray(frames)
    o = 7 + 4 + 8 + 1            # frame header, class / method, delivery tag, redelivered
    o += 1 + b[o]                # exchange
    o += 1 + b[o]                # routing key
    struct.pack_into(">I", b, o, min(int(count), 0xffffffff))
    return bytes(b)
