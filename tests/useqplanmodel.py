"""Python model of the placement plan of ma_ug_seq (reference asm.c:248-260) and of the wanted table the device readers take (host/unitig_gfa.c: ug_seq_wanted):
the yardstick of tests/test_gpu_useq_plan.py.  Unitigs are tests/ugtextmodel.py's: (len, start, end, members), members = vertex << 32 | length to the next read.

    uoff[i]    = sum over j < i of (len_j + 1), exact (Python integers); arena_bytes = uoff[U]
    per read   : (utg, start, len, ori) with start = the sum mod 2^32 of the low words of the members in front of it on its unitig -- the reference's uint32_t l
    entries    : one per read with len != 0 and a name that is not empty, ascending read id: (name, dst_off = uoff[utg] + start, len, s, e, rev, whole)

A read that is a member more than once makes the reference assert (asm.c:255); the model raises Multi, the device plan refuses."""

M32 = 0xffffffff


class Multi(Exception):
    pass


def plan(units, names, sub=None):
    """-> dict(uoff, arena_bytes, place: {read: (utg, start, len, ori)}, entries, name_bytes)"""
    uoff, tot, place = [], 0, {}
    for i, (ln, _st, _en, mem) in enumerate(units):
        uoff.append(tot)
        tot += (int(ln) & M32) + 1
        l = 0
        for m in mem:
            m = int(m)
            read = m >> 33
            if read in place:
                raise Multi(read)
            place[read] = (i, l, m & M32, m >> 32 & 1)
            l = (l + (m & M32)) & M32
    uoff.append(tot)
    entries = []
    for r in sorted(place):
        utg, start, ln, ori = place[r]
        if ln == 0 or len(names[r]) == 0:
            continue
        s, e = (0, 0) if sub is None else (int(sub["sdel"][r]) & 0x7fffffff, int(sub["e"][r]))
        entries.append((bytes(names[r]), uoff[utg] + start, ln, s, e, ori, 1 if sub is None else 0))
    return dict(uoff=uoff, arena_bytes=tot, place=place, entries=entries, name_bytes=sum(len(x[0]) for x in entries))


def wanted(entries):
    """the model's entries as Ctx.useq_place_text / Ctx.useq_stream take them"""
    return [dict(name=n, dst_off=d, len=ln, rev=bool(rev), s=s, e=None if whole else e) for n, d, ln, s, e, rev, whole in entries]
