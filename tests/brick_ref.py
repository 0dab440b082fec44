"""Reference, case tables and kernel emulation of the brick gradient exchange (csrc/brick.hip), shared by
test_brick_ref_host.py (CPU) and test_gpu_brick_exchange.py (MI355X).  Everything is compared on bits
(uint32 / uint8 / int64 views), never with `==` on floats and never with a tolerance.

Reference (``*_ref``): a numpy restatement of the four operations, written from the comment block at the top of
csrc/brick.hip and from esr_brick_list's contract -- not from the torch double (tests/brick_ops_double.py).
  flags_ref   the buffer padded with zeros to whole 128-float bricks; a brick's byte is 1 iff any value is IEEE `!= 0`:
              a subnormal flags, a NaN flags, -0.0 does not.
  list_ref    the indices of the non-zero BYTES (any non-zero byte, not only 1) ascending; the first `cap` of them, then -1
              up to `cap`; the true count even when it exceeds `cap`.
  pack_ref    slot k <- brick idx[k], the ragged last brick zero-padded; a negative idx[k] gives 128 (+0) zeros.
  unpack_ref  brick idx[k] <- slot k, truncated at n; negative slots are skipped; every other element keeps its bits.

G, the number of 32-lane groups (= bricks, = list slots) one grid-stride trip of flags / pack / unpack covers: the three
launch lines of csrc/brick.hip read ``esr_grid_for(groups * 32, 256, 256 * 16)``, i.e. ceil(groups * 32 / 256) workgroups of
256 threads, capped at 256 * 16 = 4096 workgroups.  4096 workgroups * 256 threads / 32 lanes per group = 32768 groups per
trip.  test_brick_ref_host.py reads the launch lines and fails when they change, so a changed cap cannot silently shrink the
coverage of the sizes below.  Trips per size: G - 1, G -> 1;  G + 1, G + 131 -> 2;  2G + 3 -> 3 (the last one holds 3 bricks:
an odd number, so the upper half of the last active wave is idle; so it is at G + 1, G + 131 and at nb = 33, where the
launch has 40 groups for 33 bricks).  Index lists: length 1, G -> 1 trip;  G + 1 -> 2;  2G + 5 -> 3.

Emulation (``emu_*``): the kernels' decomposition in numpy -- 32-lane groups two to a 64-lane wave with one ballot per
wave, a float4 per lane, the scalar tail of the ragged last brick lane by lane, the stride over trips, 256 chunks by 256
threads with `per` flags per thread for the list -- with a ``mut=`` argument that plants one defect (MUTANTS).  The host
test shows that the unmutated emulation passes every case and that every mutant fails a named one: the case tables can
see each of these defects, so they would see it in the HIP kernels.

Output buffers are pre-filled with the byte PAT (0xA5); what the reference leaves alone must keep it.  The emulation sees
PAT behind the end of a buffer, as the GPU test's guard bands put it there."""
import functools

import numpy as np

BRICK = 128
GROUP = 32                      # lanes per brick
BLOCK = 256                     # threads per workgroup
GRID_CAP = 256 * 16             # workgroups per launch at the most
G = GRID_CAP * BLOCK // GROUP   # 32768 groups per trip
LIST_BLOCKS = LIST_THREADS = 256
PAT = 0xA5
PAT32 = np.uint32(0xA5A5A5A5)
PAT64 = np.array([0xA5A5A5A5A5A5A5A5], np.uint64).view(np.int64)[0]
FLT_MIN = np.float32(1.17549435e-38)

SPECIALS = [            # (name, bits, flags?) -- each planted alone in an otherwise zero brick
    ("-0", 0x80000000, 0), ("+sub", 0x00000001, 1), ("-sub", 0x80000001, 1), ("+inf", 0x7F800000, 1),
    ("-inf", 0xFF800000, 1), ("nan_a", 0x7FC12345, 1), ("nan_b", 0xFF812345, 1),
]


def n_bricks(n):
    return (n + BRICK - 1) // BRICK


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))


# ------------------------------------------------------------------------------------------------ reference
def flags_ref(x):
    x = np.asarray(x, np.float32)
    nb = n_bricks(x.size)
    pad = np.zeros(nb * BRICK, np.float32)
    pad[:x.size] = x
    with np.errstate(invalid="ignore"):
        return (pad.reshape(nb, BRICK) != 0).any(1).astype(np.uint8)


def list_ref(flags, cap):
    on = np.flatnonzero(np.asarray(flags, np.uint8) != 0).astype(np.int64)
    idx = np.full(cap, -1, np.int64)
    k = min(cap, on.size)
    idx[:k] = on[:k]
    return idx, int(on.size)


def pack_ref(x, idx):
    nb = n_bricks(x.size)
    pad = np.zeros(nb * BRICK, np.uint32)
    pad[:x.size] = u32(x)
    idx = np.asarray(idx, np.int64)
    out = np.zeros((idx.size, BRICK), np.uint32)
    ok = idx >= 0
    out[ok] = pad.reshape(nb, BRICK)[idx[ok]]
    return out.reshape(-1).view(np.float32)


def unpack_ref(packed, idx, x):
    n, nb = x.size, n_bricks(x.size)
    pad = np.zeros(nb * BRICK, np.uint32)
    pad[:n] = u32(x)
    idx = np.asarray(idx, np.int64)
    ok = idx >= 0
    pad.reshape(nb, BRICK)[idx[ok]] = u32(packed).reshape(-1, BRICK)[ok]
    return pad[:n].view(np.float32)


# ------------------------------------------------------------------------------------------------ buffers
# name -> (nb, n, what the ragged last brick holds: "last" = non-zero only in its very last element, "zero" = nothing)
BUFFERS = {
    "nb1": (1, 128, None), "nb1_t5": (1, 5, "last"), "nb31": (31, 31 * 128, None), "nb32": (32, 32 * 128, None),
    "nb33": (33, 33 * 128, None), "nb33_t3": (33, 32 * 128 + 3, "last"), "nb33_t4_zero": (33, 32 * 128 + 4, "zero"),
    "G-1": (G - 1, (G - 1) * 128, None), "G": (G, G * 128, None), "G+1": (G + 1, (G + 1) * 128, None),
    "G+131": (G + 131, (G + 131) * 128, None), "2G+3": (2 * G + 3, (2 * G + 3) * 128, None),
    **{"2G+3_t%d" % t: (2 * G + 3, (2 * G + 2) * 128 + t, "last") for t in (1, 3, 4, 5, 127)},
    "2G+3_t5_zero": (2 * G + 3, (2 * G + 2) * 128 + 5, "zero"),
}


def special_bricks(nb, n):
    """{brick: (name, bits, flags?)} of the planted special values, and the one-hot blocks [(first brick, count)]"""
    whole = n // BRICK
    spec, blocks = {}, []
    if whole >= 300:
        blocks = [(5, 128), (whole - 128, 128)]                 # the first trip, and the end of the last one
        for base in (140, whole - 150):
            for j, s in enumerate(SPECIALS):
                spec[base + 2 * j] = s                          # zero bricks in between
    elif whole >= 8:
        for j, s in enumerate(SPECIALS):
            spec[1 + j] = s
    return spec, blocks


@functools.lru_cache(maxsize=None)
def buffer(name):
    """the float32 buffer of a BUFFERS entry (read-only): zero bricks, random normal bricks with zeros inside, the one-hot
    blocks (brick i of a block holds one non-zero, at position i), the special values, the ragged last brick"""
    nb, n, tail = BUFFERS[name]
    rng = np.random.default_rng(1000 + nb + n)
    whole = n // BRICK
    x = np.zeros((nb, BRICK), np.uint32)
    spec, blocks = special_bricks(nb, n)
    if whole >= 300:
        dirty = np.flatnonzero(rng.random(whole) < 0.1)
    else:
        dirty = np.array([b for b in range(whole) if b == 0 or (b >= 9 and b % 2 == 1)], np.int64)
    v = rng.standard_normal((dirty.size, BRICK)).astype(np.float32)
    v[rng.random(v.shape) < 0.3] = 0.0
    if whole < 300 and dirty.size > 1:                          # small: the odd bricks >= 9 are one-hot
        for r, b in enumerate(dirty[1:], 1):
            keep = v[r, (b * 37) % BRICK] or np.float32(1.5)
            v[r] = 0.0
            v[r, (b * 37) % BRICK] = keep
    x[dirty] = u32(v)
    for first, cnt in blocks:
        x[first:first + cnt] = 0
        x[first + np.arange(cnt), np.arange(cnt)] = u32(np.float32(1.0) + np.arange(cnt, dtype=np.float32) / 128)
    for b, (_, bits, _) in spec.items():
        x[b] = 0
        x[b, (b * 53 + 77) % BRICK] = bits
    x = x.reshape(-1)
    if n % BRICK:
        x[whole * BRICK:] = 0
        if tail == "last":
            x[n - 1] = 0x3FC00000                               # 1.5
    out = x[:n].copy().view(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def index_lists(name):
    """{list name: (idx int64, usable for unpack?)} for the buffer `name`.  Unpack lists hold no brick twice."""
    nb, n, _ = BUFFERS[name]
    rng = np.random.default_rng(77 + nb)
    last = nb - 1
    spec, blocks = special_bricks(nb, n)
    must = sorted(set(spec) | {b for f, c in blocks for b in (f, f + c - 1)} | {last})

    def distinct(m):            # m distinct bricks, the special ones and the ragged one among them
        keep = [b for b in must][:m]
        rest = np.setdiff1d(np.arange(nb), keep)
        return np.concatenate([np.array(keep, np.int64), rng.choice(rest, m - len(keep), replace=False)]).astype(np.int64)

    def put(a, slot, brick):    # move `brick` to `slot` of the duplicate-free list a
        a = a.copy()
        j = int(np.flatnonzero(a == brick)[0])
        a[j], a[slot] = a[slot], a[j]
        return a

    def holes(real, mask):      # the entries `real` in the slots where mask is False, -1 elsewhere
        a = np.full(mask.size, -1, np.int64)
        a[~mask] = real
        return a

    out = {"one_last": (np.array([last], np.int64), True)}
    if nb <= 64:
        out["asc_all"] = (np.arange(nb, dtype=np.int64), True)
        out["perm_all"] = (rng.permutation(nb).astype(np.int64), True)
        a = []
        for b in range(nb):                                     # a -1 behind every even brick, two trailing ones
            a += [b, -1] if b % 2 == 0 else [b]
        out["asc_neg"] = (np.array(a + [-1, -1], np.int64), True)
        out["all_neg"] = (np.full(5, -1, np.int64), True)
        d = rng.integers(-1, nb, nb + 9).astype(np.int64)
        d[2] = d[-1] = last
        out["dups"] = (d, False)
    elif nb > 2 * G:
        out["asc_G"] = (np.sort(distinct(G)), True)                            # the ragged brick in the last slot
        out["perm_G1"] = (put(rng.permutation(distinct(G + 1)), 3, last), True)  # two trips, the second one group
        L = 2 * G + 5
        mask = np.arange(L) % 5 == 1                                           # interleaved -1 ...
        mask[-3:] = True                                                       # ... and trailing ones
        m = int((~mask).sum())
        out["asc_2G5_neg"] = (holes(np.sort(distinct(m)), mask), True)         # the ragged brick in slot 2G + 1: last trip
        out["perm_2G5_neg"] = (holes(put(rng.permutation(distinct(m)), 3, last), mask), True)   # ... in the first trip
        out["all_neg"] = (np.full(G + 1, -1, np.int64), True)
        d = rng.integers(-1, nb, L).astype(np.int64)
        d[3] = d[-1] = last
        out["dups"] = (d, False)
    for k, (a, _) in out.items():
        a.setflags(write=False)
    return out


def packed_bits(n_idx, seed):
    """what unpack scatters: arbitrary bit patterns (NaN payloads, subnormals, -0 among them)"""
    return np.random.default_rng(seed).integers(0, 2 ** 32, n_idx * BRICK, dtype=np.uint64).astype(np.uint32).view(np.float32)


MOVE_BUFFERS_ALL_LISTS = ("nb33_t3", "2G+3_t5")


def cases():
    """every case id, in the order small to large: 'flags/<buffer>', 'pack/<buffer>/<list>', 'unpack/<buffer>/<list>',
    'list/nb<nb>/<density>/<cap>' and 'list2/...' (a second call on the same scratch buffer with other flags)"""
    out = []
    for name in BUFFERS:
        out.append("flags/" + name)
    for name, (nb, n, tail) in BUFFERS.items():
        if name in MOVE_BUFFERS_ALL_LISTS:
            lists = list(index_lists(name))
        elif n % BRICK or nb <= 33:
            lists = ["one_last"]
        else:
            continue
        for l in lists:
            out.append("pack/%s/%s" % (name, l))
            if index_lists(name)[l][1]:
                out.append("unpack/%s/%s" % (name, l))
    out.sort(key=lambda c: BUFFERS[c.split("/")[1]][0] > 64)
    for nb in LIST_NB:
        for dens in LIST_DENSITIES:
            for cap in list_caps(nb, dens):
                out.append("list/nb%d/%s/%s" % (nb, dens, cap))
    out.append("list2/nb257/0.3/count")
    return out


LIST_NB = (1, 255, 256, 257, 65535, 65536, 65537)
LIST_DENSITIES = ("0", "1", "0.3")


@functools.lru_cache(maxsize=None)
def list_flags(nb, dens, salt=0):
    rng = np.random.default_rng(nb * 7 + salt)
    on = {"0": np.zeros(nb, bool), "1": np.ones(nb, bool)}.get(dens)
    if on is None:
        on = rng.random(nb) < float(dens)
    f = np.where(on, rng.choice(np.array([1, 2, 255], np.uint8), nb), 0).astype(np.uint8)
    f.setflags(write=False)
    return f


def list_caps(nb, dens):
    """labels of the capacities of one flag set: 0 (with a NULL idx), count - 1, count, count + 1, nb"""
    count = int((list_flags(nb, dens) != 0).sum())
    seen, out = set(), []
    for label, cap in (("0", 0), ("count-1", count - 1), ("count", count), ("count+1", count + 1), ("nb", nb)):
        if cap >= 0 and cap not in seen:
            seen.add(cap)
            out.append(label)
    return out


def list_cap(nb, dens, label, salt=0):
    count = int((list_flags(nb, dens, salt) != 0).sum())
    return {"0": 0, "count-1": count - 1, "count": count, "count+1": count + 1, "nb": nb}[label]


class Scratch:
    """what lives between two esr_brick_list calls: the 256 chunk counts"""
    def __init__(self):
        self.counts = np.full(LIST_BLOCKS, 0x5A5A5A5A, np.int32)


def run_case(impl, case, scratch=None):
    """None when `impl` (flags(x) -> uint8 [nb]; pack(x, idx) -> float32; unpack(packed, idx, x) -> (x', what lies behind
    x' or None); list(flags, cap, scratch) -> (idx, count)) gives the reference's bits on `case`, else what differs."""
    kind, *arg = case.split("/")
    if kind == "flags":
        x = buffer(arg[0])
        got = impl.flags(x)
        return None if same_bits(got, flags_ref(x)) else "flags differ at bricks %s" % _where(got, flags_ref(x))
    if kind in ("pack", "unpack"):
        x = buffer(arg[0])
        idx = index_lists(arg[0])[arg[1]][0]
        if kind == "pack":
            got, want = impl.pack(x, idx), pack_ref(x, idx)
            return None if same_bits(got, want) else "packed differs at floats %s" % _where(u32(got), u32(want))
        packed = packed_bits(idx.size, 5 + idx.size)
        got, behind = impl.unpack(packed, idx, x)
        want = unpack_ref(packed, idx, x)
        if behind is not None and not bool((u32(behind) == PAT32).all()):
            return "unpack wrote behind the end of the buffer"
        return None if same_bits(got, want) else "buffer differs at floats %s" % _where(u32(got), u32(want))
    nb, dens, label = int(arg[0][2:]), arg[1], arg[2]
    scratch = scratch or Scratch()
    if kind == "list2":                    # a call with other flags first, on the same scratch
        impl.list(list_flags(nb, "1"), nb, scratch)
    salt = 1 if kind == "list2" else 0
    flags, cap = list_flags(nb, dens, salt), list_cap(nb, dens, label, salt)
    idx, count = impl.list(flags, cap, scratch)
    want_idx, want_count = list_ref(flags, cap)
    if int(count) != want_count:
        return "count %d, expected %d" % (int(count), want_count)
    return None if same_bits(np.asarray(idx, np.int64), want_idx) else "idx differs at slots %s" % _where(idx, want_idx)


def _where(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return "(shapes %s, %s)" % (a.shape, b.shape)
    w = np.flatnonzero(a != b)
    return "%s (%d in all)" % (w[:4].tolist(), w.size)


# ------------------------------------------------------------------------------------------------ emulation
MOVE = ("flags", "pack", "unpack")
MUTANTS = {             # name: (the operations it changes -- each must reject it, what it does)
    "no_stride": (MOVE, "the stride over trips drops every brick / slot >= G"),
    "upper_from_lower": (("flags",), "the upper half-wave's ballot is taken from the lower half"),
    "no_tail": (MOVE, "the scalar tail of the ragged brick is skipped"),
    "tail_plus_one": (MOVE, "the scalar tail reads / writes one element past n"),
    "pack_skip_neg": (("pack",), "pack leaves a -1 slot unwritten"),
    "unpack_neg_to_0": (("unpack",), "unpack writes a -1 slot to brick 0"),
    "negzero_flags": (("flags",), "-0.0 flags (a compare on bits)"),
    "subnormal_noflag": (("flags",), "a subnormal does not flag (denormals flushed)"),
    "list_chunk_edge": (("list",), "the count pass misses a chunk's last flag: ranks are off by one behind that chunk boundary"),
    "list_no_fill": (("list",), "the slots [count, cap) stay unwritten"),
    "count_saturates": (("list",), "the count saturates at cap"),
    "list_byte_is_one": (("list",), "only a flag byte of 1 counts"),
}


def _launch_groups(groups):
    grid = min(max((groups * GROUP + BLOCK - 1) // BLOCK, 1), GRID_CAP)        # esr_grid_for(groups * 32, 256, 256 * 16)
    return grid * BLOCK // GROUP


def _nonzero(v, mut):
    with np.errstate(invalid="ignore"):
        if mut == "negzero_flags":
            return u32(v) != 0
        if mut == "subnormal_noflag":
            return (v != 0) & ~(np.abs(v) < FLT_MIN)
        return v != 0


def emu_flags(x, mut=None):
    n, nb = x.size, n_bricks(x.size)
    mem = np.concatenate([u32(x), np.full(BRICK, PAT32, np.uint32)]).view(np.float32)      # PAT lies behind the buffer
    flags = np.full(nb, PAT, np.uint8)
    if n == 0:
        return flags
    ngrp, whole = _launch_groups(nb), n // BRICK
    lanes = mem[:whole * BRICK].reshape(whole, GROUP, 4)
    for b0 in range(0, nb, ngrp):                                       # one trip of the grid-stride loop
        if mut == "no_stride" and b0 > 0:
            break
        bs = b0 + np.arange(ngrp)
        act = bs < nb
        nz = np.zeros((ngrp, GROUP), bool)                              # a lane that left the loop gives a 0 ballot bit
        full = act & (bs < whole)
        nz[full] = _nonzero(lanes[bs[full]], mut).any(2)                # one float4 per lane
        for g in np.flatnonzero(act & ~full):                           # the ragged last brick, lane by lane
            for sub in range(GROUP):
                e = int(bs[g]) * BRICK + sub * 4
                if e + 4 <= n:
                    nz[g, sub] = _nonzero(mem[e:e + 4], mut).any()
                elif mut != "no_tail":
                    for i in range(e, n + 1 if mut == "tail_plus_one" else n):
                        nz[g, sub] |= bool(_nonzero(mem[i:i + 1], mut)[0])
        half = nz.reshape(ngrp // 2, 2, GROUP).any(2)                   # the wave's ballot, one 32-bit half per group
        if mut == "upper_from_lower":
            half[:, 1] = half[:, 0]
        flags[bs[act]] = half.reshape(ngrp)[act]
    return flags


def _emu_move(unpack, x, idx, packed, mut):
    n, n_idx = x.size, idx.size
    mem = np.concatenate([u32(x), np.full(BRICK, PAT32, np.uint32)])
    pk = u32(packed).copy().reshape(n_idx, BRICK)
    if n_idx == 0:
        return mem, pk
    ngrp, whole = _launch_groups(n_idx), n // BRICK
    bricks = mem[:whole * BRICK].reshape(whole, BRICK)
    for k0 in range(0, n_idx, ngrp):
        if mut == "no_stride" and k0 > 0:
            break
        ks = np.arange(k0, min(k0 + ngrp, n_idx))
        b = idx[ks].copy()
        neg = b < 0
        if unpack and mut == "unpack_neg_to_0":
            b[neg], neg = 0, np.zeros_like(neg)
        if not unpack and mut != "pack_skip_neg":
            pk[ks[neg]] = 0
        full = ~neg & (b < whole)
        if unpack:
            bricks[b[full]] = pk[ks[full]]                              # one float4 per lane, 32 lanes per brick
        else:
            pk[ks[full]] = bricks[b[full]]
        for j in np.flatnonzero(~neg & ~full):                          # the ragged last brick, lane by lane
            k, bb = int(ks[j]), int(b[j])
            for sub in range(GROUP):
                e, p = bb * BRICK + sub * 4, sub * 4
                if e + 4 <= n:
                    if unpack:
                        mem[e:e + 4] = pk[k, p:p + 4]
                    else:
                        pk[k, p:p + 4] = mem[e:e + 4]
                elif mut != "no_tail":
                    lim = n + 1 if mut == "tail_plus_one" else n
                    if unpack:
                        for i in range(4):
                            if e + i < lim:
                                mem[e + i] = pk[k, p + i]
                    else:
                        t = [0, 0, 0, 0]
                        for i in range(4):
                            if e + i < lim:
                                t[i] = mem[e + i]
                        pk[k, p:p + 4] = t
    return mem, pk


def emu_pack(x, idx, mut=None):
    packed = np.full(idx.size * BRICK, PAT32, np.uint32).view(np.float32)
    return _emu_move(False, x, idx, packed, mut)[1].reshape(-1).view(np.float32)


def emu_unpack(packed, idx, x, mut=None):
    mem, _ = _emu_move(True, x, idx, packed, mut)
    return mem[:x.size].view(np.float32), mem[x.size:]


def emu_list(flags, cap, scratch, mut=None):
    nb = flags.size
    on = (flags == 1) if mut == "list_byte_is_one" else (flags != 0)
    csum = np.concatenate([[0], np.cumsum(on)]).astype(np.int64)
    chunk = (nb + LIST_BLOCKS - 1) // LIST_BLOCKS
    per = (chunk + LIST_THREADS - 1) // LIST_THREADS
    t = np.arange(LIST_THREADS)

    def ranges(c, short=0):
        b0 = c * chunk
        e0 = min(b0 + chunk, nb)
        e0 = max(b0, e0 - short) if e0 > b0 else e0
        lo = np.minimum(b0 + t * per, e0)
        return lo, np.minimum(lo + per, e0)

    counts = scratch.counts
    for c in range(LIST_BLOCKS):                                        # pass 1: flagged bricks per chunk
        lo, hi = ranges(c, short=1 if mut == "list_chunk_edge" else 0)
        counts[c] = int((csum[hi] - csum[lo]).sum())
    idx = np.full(cap, PAT64, np.int64)
    ex = np.cumsum(counts) - counts                                     # pass 2: every workgroup scans the chunk counts
    total = int(counts.sum())
    for c in range(LIST_BLOCKS):
        lo, hi = ranges(c)
        mine = csum[hi] - csum[lo]
        r = ex[c] + np.cumsum(mine) - mine                              # rank of each thread's first flagged brick
        for j in range(per):                                            # thread t walks lo .. hi
            i = lo + j
            ok = i < hi
            hit = ok & on[np.minimum(i, nb - 1)] if nb else ok & False
            rank = r + (csum[np.minimum(i, nb)] - csum[lo])
            w = hit & (rank < cap)
            idx[rank[w]] = i[w]
    if mut != "list_no_fill" and total < cap:
        idx[total:cap] = -1
    return idx, (min(total, cap) if mut == "count_saturates" else total)


class Emu:
    """run_case's `impl` on the emulation"""
    def __init__(self, mut=None):
        self.mut = mut

    def flags(self, x):
        return emu_flags(x, self.mut)

    def pack(self, x, idx):
        return emu_pack(x, idx, self.mut)

    def unpack(self, packed, idx, x):
        return emu_unpack(packed, idx, x, self.mut)

    def list(self, flags, cap, scratch):
        return emu_list(flags, cap, scratch, self.mut)


# ------------------------------------------------------------------------------------------------ two ranks
# One GridGradSync per letter runs its steps in order, so each step's capacity is the one learnt from the step before:
# capacity' = max(min_capacity, int(union * 1.25)); a step sends min(capacity, bricks) slots, and union - capacity more in
# verify() when the union outgrew it.  `sent`, `overflow` and `mode` below are written out by hand from that rule.
NB_A = 3001
N_A = NB_A * BRICK - 51
SYNCS = {
    "A": dict(min_capacity=1),                                          # dense_above = 0.8: never reached below
    "B": dict(min_capacity=1, dense_above=0.1),
    "C": dict(min_capacity=2 * G + 1, dense_above=2.0),                 # a list of 2G + 1 slots over 2G + 3 bricks
    "D": dict(min_capacity=1, dense_above=2.0),                         # (one brick of one is "dense" otherwise)
}


def _pick(rng, pool, m):
    return np.sort(rng.choice(pool, m, replace=False))


@functools.lru_cache(maxsize=None)
def scenarios():
    """[dict(name, sync, n, sets=(bricks of rank 0, bricks of rank 1), cancel=bricks where a1 == -a0, mode, union, bricks, sent,
    overflow)] -- the steps of the two-rank scenario table in the order they run"""
    rng = np.random.default_rng(2024)
    allb = np.arange(NB_A)
    last = NB_A - 1
    none = np.zeros(0, np.int64)
    out = []

    def add(name, sync, n, s0, s1, mode, sent, overflow=0, cancel=none):
        s0, s1 = np.asarray(s0, np.int64), np.asarray(s1, np.int64)
        out.append(dict(name=name, sync=sync, n=n, sets=(s0, s1), cancel=np.asarray(cancel, np.int64), mode=mode,
                        union=int(np.union1d(s0, s1).size), bricks=n_bricks(n), sent=sent, overflow=overflow, seed=len(out)))

    add("1 disjoint", "A", N_A, _pick(rng, allb[0::2], 150), _pick(rng, allb[1::2], 150), "sparse", 300)     # first step: exact
    stu = _pick(rng, allb, 300)
    add("2 overlapping", "A", N_A, stu[:200], stu[100:], "sparse", 375)                                      # 300 * 1.25
    add("3 rank 1 all zero", "A", N_A, _pick(rng, allb, 250), none, "sparse", 375)
    s4 = np.union1d(_pick(rng, allb[:-1], 199), [last])
    add("4 a0 == -a1", "A", N_A, s4, s4[-120:], "sparse", 312, cancel=s4[-40:])                            # 250 * 1.25; ragged brick cancels
    add("5 the same again", "A", N_A, s4, s4[-120:], "sparse", 250, cancel=s4[-40:])                        # 50 trailing -1 slots
    s6 = _pick(rng, allb, 400)
    add("6 grows", "A", N_A, s6, s6, "sparse", 400, overflow=150)                                          # capacity 250
    add("7 shrinks", "A", N_A, _pick(rng, allb, 25), _pick(rng, allb, 25)[:15], "sparse", 500)
    s8 = _pick(rng, allb, 600)
    add("8 dense, first step", "B", N_A, s8[:400], s8[200:], "dense", NB_A)
    add("8 dense, by capacity", "B", N_A, s8[100:], s8[:300], "dense", NB_A)
    nb9 = 2 * G + 3
    big = np.arange(nb9)
    add("9 2G+3 bricks, first step", "C", (nb9 - 1) * BRICK + 5, np.union1d(_pick(rng, big, 7000), [nb9 - 1]), _pick(rng, big, 7000),
        "sparse", None)                                                                                     # exact: sent == union
    add("9 2G+3 bricks, three trips", "C", (nb9 - 1) * BRICK + 5, np.union1d(_pick(rng, big, 7000), [nb9 - 1]), _pick(rng, big, 7000),
        "sparse", 2 * G + 1)
    add("10 n < 128, first step", "D", 77, [0], [0], "sparse", 1)
    add("10 n < 128", "D", 77, [0], none, "sparse", 1)
    for s in out:
        if s["sent"] is None:
            s["sent"] = s["union"]
    return out


def rank_buffer(sc, rank):
    """the flat gradient of `rank` in step `sc`: +0 outside its bricks; inside, normal numbers of either sign in
    [0.5, 1.5) with a quarter of the elements +0; on the cancel bricks rank 1 holds rank 0's values negated"""
    def fill(r):
        rng = np.random.default_rng(10_000 + 10 * sc["seed"] + r)
        nb = sc["bricks"]
        x = np.zeros((nb, BRICK), np.float32)
        s = sc["sets"][r]
        v = ((0.5 + rng.random((s.size, BRICK))) * rng.choice([-1.0, 1.0], (s.size, BRICK))).astype(np.float32)
        v[rng.random(v.shape) < 0.25] = 0.0
        x[s] = v
        return x
    x = fill(rank)
    if rank == 1 and sc["cancel"].size:
        x[sc["cancel"]] = -fill(0)[sc["cancel"]]
        x[sc["cancel"]] += np.float32(0.0)                      # (-(+0) is -0: the inputs hold +0 zeros only)
    return np.ascontiguousarray(x.reshape(-1)[:sc["n"]])


def run_two_rank(rank, device, make_sync, say=print):
    """the scenario table on this rank; `make_sync(**kw)` builds a GridGradSync over the two-rank group.  Asserts, after
    reduce() and verify(), that the buffer holds the bits of a0 + a1 (float32, added on the CPU), and `last`."""
    import torch
    cuda = str(device).startswith("cuda")
    syncs = {}
    for sc in scenarios():
        a0, a1 = rank_buffer(sc, 0), rank_buffer(sc, 1)
        assert not (np.signbit(a0) & (a0 == 0)).any() and not (np.signbit(a1) & (a1 == 0)).any()
        want = torch.from_numpy(a0) + torch.from_numpy(a1)
        flat = torch.from_numpy((a0, a1)[rank].copy()).to(device)
        if sc["sync"] not in syncs:
            syncs[sc["sync"]] = make_sync(**SYNCS[sc["sync"]])
        sync = syncs[sc["sync"]]
        sync.reduce(flat)
        if cuda:
            torch.cuda.synchronize()
        if sc["overflow"]:                                      # the overflowing bricks are still this rank's own
            assert not torch.equal(flat.cpu().view(torch.int32), want.view(torch.int32)), (sc["name"], "exact before verify()")
        sync.verify()
        if cuda:
            torch.cuda.synchronize()
        got = flat.cpu()
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero().view(-1)
        assert bad.numel() == 0, (sc["name"], "rank", rank, "wrong bits at", bad[:8].tolist(), "of", bad.numel())
        last = sync.last
        assert last["mode"] == sc["mode"] and last["union"] == sc["union"] and last["bricks"] == sc["bricks"], (sc["name"], last)
        assert last["sent"] == sc["sent"] and last["sent"] >= last["union"], (sc["name"], last)
        assert last.get("overflow", 0) == sc["overflow"], (sc["name"], last)
        say("BRICKX %-28s %s" % (sc["name"], last))


WORKER = r'''
import os, sys, time
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch, torch.distributed as dist
import brick_ref as R
from esr_nerf_amd.grad_sync import GridGradSync
rank, device = int(os.environ["RANK"]), sys.argv[2]
dist.init_process_group("gloo")
ops = None                                      # the product's default: HipBrickOps
if device == "cpu":
    from brick_ops_double import TorchBrickOps
    ops = TorchBrickOps()
else:
    torch.cuda.set_device(0)
t0 = time.time()
R.run_two_rank(rank, device, lambda **kw: GridGradSync(dist.group.WORLD, ops=ops, **kw),
               say=print if rank == 0 else (lambda *a: None))
dist.barrier()
if rank == 0:
    print("BRICKX done %.1f s" % (time.time() - t0))
dist.destroy_process_group()
'''
