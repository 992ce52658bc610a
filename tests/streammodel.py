"""A model of the persistent name table of the streamed PAF ingest (csrc/paf.hip: stream_hash, k_stream_fold, k_stream_rebuild), in numpy and plain Python, so
that a test can CHOOSE names by where the table puts them: stream_hash(name) = key_mix(fnv1a64(name)); home slot = low 32 bits & (cap - 1); tag = high 32 bits;
linear probing, at most PROBE_LIMIT slots a name.  A pool of fixed-width names `c%07d` is hashed once per process (about a second for 1.5 M names); from it come
names whose home lies in a narrow window of a table (they crowd one chain until a probe sequence runs out), pairs of names with the same tag and home, and names
whose home is the last slot.  Every case asserts with simulate() that its names do what it needs before it touches the device."""
import numpy as np

FNV_OFF, FNV_PRIME = 0xcbf29ce484222325, 0x100000001b3
PROBE_LIMIT = 2048  # paf.hip: PAF_PROBE_LIMIT
EMPTY = 0xFFFFFFFFFFFFFFFF  # paf.hip: PAF_EMPTY
PROV = 0x80000000  # paf.hip: ST_PROV
M64 = (1 << 64) - 1
POOL_N = 1500000


def key_mix(z):
    z ^= z >> 33
    z = z * 0xff51afd7ed558ccd & M64
    z ^= z >> 33
    z = z * 0xc4ceb9fe1a85ec53 & M64
    z ^= z >> 33
    return z


def stream_hash(name):
    h = FNV_OFF
    for b in bytes(name):
        h = (h ^ b) * FNV_PRIME & M64
    return key_mix(h)


def home(name, cap):
    return stream_hash(name) & 0xFFFFFFFF & (cap - 1)


def tag(name):
    return stream_hash(name) >> 32


def hash_many(names):
    """stream_hash of an (n, width) uint8 array of names of one width, vectorised (uint64 arithmetic wraps as the device's does)"""
    names = np.ascontiguousarray(names, dtype=np.uint8)
    with np.errstate(over="ignore"):
        h = np.full(len(names), FNV_OFF, dtype=np.uint64)
        for k in range(names.shape[1]):
            h = (h ^ names[:, k].astype(np.uint64)) * np.uint64(FNV_PRIME)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xc4ceb9fe1a85ec53)
        h ^= h >> np.uint64(33)
    return h


_POOL = {}


def pool():
    """(hashes, name(i)) of the names c0000000 .. c1499999, hashed once"""
    if "h" not in _POOL:
        idx = np.arange(POOL_N, dtype=np.int64)
        a = np.empty((POOL_N, 8), dtype=np.uint8)
        a[:, 0] = ord("c")
        for k in range(7):
            a[:, 7 - k] = ord("0") + (idx // 10 ** k) % 10
        _POOL["h"] = hash_many(a)
    return _POOL["h"]


def pool_name(i):
    return b"c%07d" % int(i)


def clustered(cap, window=64):
    """the pool's names whose home lies in slots [0, window) of a table of `cap` slots, in pool order"""
    h = pool()
    return [pool_name(i) for i in np.flatnonzero((h & np.uint64(0xFFFFFFFF) & np.uint64(cap - 1)) < np.uint64(window))]


def equal_tag_pairs(cap):
    """pairs of pool names with the same tag and the same home in a table of `cap` slots"""
    h = pool()
    t = h >> np.uint64(32)
    order = np.argsort(t, kind="stable")
    ts = t[order]
    out = []
    for k in np.flatnonzero(ts[1:] == ts[:-1]):
        a, b = int(order[k]), int(order[k + 1])
        if (int(h[a]) ^ int(h[b])) & 0xFFFFFFFF & (cap - 1) == 0:
            out.append((pool_name(a), pool_name(b)))
    return out


def with_home(slot, cap, n):
    """the first n pool names whose home in a table of `cap` slots is `slot`"""
    h = pool()
    return [pool_name(i) for i in np.flatnonzero((h & np.uint64(0xFFFFFFFF) & np.uint64(cap - 1)) == np.uint64(slot))[:n]]


class Table:
    """the table: linear probing over `cap` slots, at most `limit` probes; slots hold (name, id) or None"""

    def __init__(self, cap, limit=PROBE_LIMIT):
        self.cap, self.limit, self.slots, self.where = cap, limit, [None] * cap, {}

    def insert(self, name, gid):
        """-> the number of slots probed, or None when the sequence runs out (nothing is stored then)"""
        s = home(name, self.cap)
        for k in range(self.limit):
            at = (s + k) & (self.cap - 1)
            if self.slots[at] is None:
                self.slots[at], self.where[name] = (name, gid), at
                return k + 1
            if self.slots[at][0] == name:
                return k + 1
        return None

    def displacement(self, name):
        return (self.where[name] - home(name, self.cap)) & (self.cap - 1)


def simulate(names, cap, limit=PROBE_LIMIT, reverse=False):
    """the names (distinct, ids = their positions) inserted in the given or the reversed order -> (table, names whose sequence ran out)"""
    t, out = Table(cap, limit), []
    order = list(enumerate(names))
    for gid, nm in (reversed(order) if reverse else order):
        if t.insert(nm, gid) is None:
            out.append(nm)
    return t, out


def overflows(names, cap, limit=PROBE_LIMIT):
    """does inserting these names overflow a probe sequence, under forward AND reversed insertion order?  -> (forward, reversed)"""
    return bool(simulate(names, cap, limit)[1]), bool(simulate(names, cap, limit, True)[1])


def check_device_table(slots, names, limit=PROBE_LIMIT):
    """slots: the downloaded table (uint64 per slot); names: the stream's names by id.  Every occupied slot holds tag << 32 | id of a name whose probe sequence
    reaches it with only occupied slots on the way; every id sits in exactly one slot; no slot holds a provisional word.  -> the number of occupied slots"""
    cap = len(slots)
    assert cap & (cap - 1) == 0
    occ = np.flatnonzero(slots != np.uint64(EMPTY))
    seen = set()
    for s in occ:
        w = int(slots[s])
        gid, tg = w & 0xFFFFFFFF, w >> 32
        assert not gid & PROV, "slot %d holds a provisional word %#x between pieces" % (s, w)
        assert gid < len(names), "slot %d holds id %d of %d" % (s, gid, len(names))
        nm = names[gid]
        assert tg == tag(nm), "slot %d: tag %#x, the name %r has %#x" % (s, tg, nm, tag(nm))
        d = (int(s) - home(nm, cap)) & (cap - 1)
        assert d < limit, "slot %d lies %d slots behind the home of %r" % (s, d, nm)
        h = home(nm, cap)
        assert all(slots[(h + k) & (cap - 1)] != np.uint64(EMPTY) for k in range(d)), "a free slot between the home of %r and its slot %d: a lookup would miss it" % (nm, s)
        assert gid not in seen, "id %d sits in two slots" % gid
        seen.add(gid)
    assert len(seen) == len(names), "%d ids in the table, %d names" % (len(seen), len(names))
    return len(occ)
