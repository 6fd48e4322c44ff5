"""gpu tier: the radix sort, its spine and the scans in every form the library uses them in (csrc/radix_sort.h: radix_sort_pairs
with begin_bit, check_from_bit and RsSeg, radix_spine; csrc/scan.h: device_scan exclusive / inclusive / in place,
device_scan_with_total, RunHeadIn, device_scan_pair_bounded, ascending_offsets_kernel).

Everything goes through the debug entry points east_hip_debug_radix_sort_ex, _radix_spine, _scan_ex, _run_heads,
_scan_pair_bounded and _ascending_offsets, which call the functions the build and the consumers call -- the segments' tables
come from rs_seg_make, the spine's choice of kernels from radix_spine.  The witness is tests/sort_exact.py (pinned to
brute-force restatements by tests/test_sort_exact_host.py).  Every comparison is np.array_equal, bit for bit; every output
comes back with a guard behind it that must still hold the 0xEE it was filled with.

The tile, group and shard geometry comes from the library (geometry_out), never from constants here; the case generators
below are functions of it, and tests/test_sort_exact_host.py asserts at the default geometry what each was written to
contain, so that a generator that drifts fails without a GPU.
"""
import collections
import ctypes

import numpy as np
import pytest

import sort_exact

pytestmark = pytest.mark.gpu

_u32p, _u64p, _i64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)
ERR_INVALID = -2
EE32, EE64 = 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE

Geometry = collections.namedtuple("Geometry", "tile group total_shards spine_doc_groups spine_held_groups scan_tile scan_raw_tiles guard spine_parts")


# ---- the case generators (no GPU needed) ------------------------------------------------------------------------------------
def flat_sizes(geo):
    """256 is a wave's share of a scatter tile; the tile counts around 8 meet the XCD tile order and its empty workgroups,
    the group counts around the number of shards the shards of the totals."""
    T, G = geo.tile, geo.group * geo.tile
    return [1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 7 * T, 8 * T, 9 * T, 9 * T + 1, G - 1, G, G + 1, geo.total_shards * G + 1, 17 * T + 3]


def bit_ranges(dtype):
    """(dtype, bits, begin_bit)"""
    r = [(1, 0), (8, 0), (9, 0), (13, 5), (17, 16), (32, 24), (32, 31)]
    if np.dtype(dtype).itemsize == 8:
        r += [(40, 8), (64, 56), (64, 0)]
    return [(dtype, bits, begin_bit) for bits, begin_bit in r]


def compose(field, dtype, bits, begin_bit, rng):
    """Keys that hold `field` in the bits [begin_bit, bits) and random bits everywhere else."""
    dtype, width = np.dtype(dtype), bits - begin_bit
    n = field.size
    noise = (rng.integers(0, 1 << 32, size=n, dtype=np.uint64) << np.uint64(32)) | rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    inside = np.uint64((((1 << width) - 1) << begin_bit) & 0xFFFFFFFFFFFFFFFF)
    assert width == 64 or int(field.max()) < 1 << width
    return ((noise & ~inside) | (field.astype(np.uint64) << np.uint64(begin_bit))).astype(dtype)


def random_field(n, width, rng):
    """Uniform over the range, half of the elements set to one value at random positions: stability shows only in ties."""
    if width == 64:
        field = (rng.integers(0, 1 << 32, size=n, dtype=np.uint64) << np.uint64(32)) | rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    else:
        field = rng.integers(0, 1 << width, size=n, dtype=np.uint64)
    if n > 100:
        field[rng.integers(0, n, size=n // 2)] = field[0]
    return field


def make_keys(stream, dtype, bits, begin_bit, rng):
    """Keys whose FIRST pass meets the digits of `stream` in input order: the stream in the lowest digit of the range, a few
    random values in the digits above it (ties for the later passes), random bits outside the range."""
    width = bits - begin_bit
    field = stream & np.uint64((1 << min(width, 8)) - 1)
    if width > 8:
        field = field | (rng.integers(0, min(1 << (width - 8), 4), size=stream.size, dtype=np.uint64) << np.uint64(8))
    if width >= 18:
        field = field | (rng.integers(0, 3, size=stream.size, dtype=np.uint64) << np.uint64(width - 2))
    return compose(field, dtype, bits, begin_bit, rng)


DISTRIBUTIONS = ("equal", "ascending", "descending", "mod256", "runs64", "runs64_shifted", "all_but_one", "switch_at_tile_and_group",
                 "alternating", "uniform")


def digit_stream(name, n, geo, rng):
    """The digits the first pass of a sort meets, in input order (uint64 below 256)."""
    T, G = geo.tile, geo.group * geo.tile
    i = np.arange(n, dtype=np.uint64)
    if name == "equal":
        d = np.full(n, 0xA7, dtype=np.uint64)
    elif name == "ascending":
        d = (i * np.uint64(256)) // np.uint64(n)
    elif name == "descending":
        d = np.uint64(255) - (i * np.uint64(256)) // np.uint64(n)
    elif name == "mod256":
        d = i % np.uint64(256)
    elif name == "runs64":              # a whole wavefront on one bin, all lanes active ...
        d = ((i // np.uint64(64)) * np.uint64(37)) % np.uint64(256)
    elif name == "runs64_shifted":      # ... and the same one element on: a wavefront that holds the end of one run and the start of the next
        d = (((i + np.uint64(63)) // np.uint64(64)) * np.uint64(37)) % np.uint64(256)
    elif name == "all_but_one":
        d = np.full(n, 0x40, dtype=np.uint64)
        d[int(rng.integers(0, n))] = 0x3F
    elif name == "switch_at_tile_and_group":
        d = np.where(i < T, 9, np.where(i < G, 200, 10)).astype(np.uint64)
    elif name == "alternating":
        d = np.where(i % np.uint64(2) == 0, 0xFF, 0x00).astype(np.uint64)
    else:
        assert name == "uniform"
        d = rng.integers(0, 256, size=n, dtype=np.uint64)
    return d


def document_lengths(geo, n_docs):
    """Document lengths of a segmented sort in a fixed shuffled order.  big * G + 1 is the first length whose spine is the
    column-parallel kernel; both spine kernels run in the same pass.  6 documents: a row of totals per shard; 11: one row."""
    T, G, big = geo.tile, geo.group * geo.tile, geo.spine_doc_groups
    every = [1, 2, 63, T - 1, T, T + 1, G, G + 1, 3 * G + 5, big * G, big * G + 1]
    lengths = every if n_docs >= len(every) else [63, T + 1, G + 1, 3 * G + 5, big * G, big * G + 1][:n_docs]
    assert len(lengths) == n_docs
    order = np.random.default_rng(n_docs).permutation(n_docs)
    return [lengths[k] for k in order]


def small_document_lengths():
    """300 documents of 1 .. 3 pairs: nearly every tile of the sort is virtual."""
    return [1 + k % 3 for k in range(300)]


def spine_flat_groups(geo):
    """The parts of the column-parallel kernel (32) and the switch of its code path (2 048 against 2 049 groups)."""
    parts, held = geo.spine_parts, geo.spine_held_groups
    return [1, parts - 1, parts, parts + 1, held - 1, held, held + 1, held + 2, 5000]


SPINE_KINDS = ("multinomial", "one_digit", "digit_absent")


def spine_table(kind, n_groups, n_docs, shards, pairs, rng, doc_group0=None):
    """(group_sum[n_groups][256], digit_total[n_docs * shards][256]): every group holds `pairs` pairs, a document's totals are
    its groups' sums split at random over its shard rows (the spine must add all rows)."""
    p = rng.dirichlet(np.full(256, 0.3))
    if kind == "one_digit":
        p = np.zeros(256)
        p[200] = 1.0
    elif kind == "digit_absent":
        p[17] = 0.0
        p /= p.sum()
    else:
        assert kind == "multinomial"
    group_sum = rng.multinomial(pairs, p, size=n_groups).astype(np.uint32)
    doc_group0 = [0, n_groups] if doc_group0 is None else doc_group0
    total = np.zeros((n_docs * shards, 256), dtype=np.uint32)
    for d in range(n_docs):
        col = group_sum[doc_group0[d]:doc_group0[d + 1]].sum(axis=0, dtype=np.uint64)
        w = rng.random((shards, 256)) + 1e-3
        part = np.floor(col[None, :] * (w / w.sum(axis=0))[:-1]).astype(np.uint64)
        rows = np.concatenate([part, (col - part.sum(axis=0, dtype=np.uint64))[None, :]])
        total[d * shards:(d + 1) * shards] = rows.astype(np.uint32)
    return group_sum, total


def scan_sizes(geo):
    """1 024 is a wave's share of a tile; raw_tiles tiles is the most whose sums the apply kernel adds up itself."""
    S, R = geo.scan_tile, geo.scan_raw_tiles
    return [1, 3, 4, 5, 1023, 1024, 1025, S - 1, S, S + 1, 2 * S + 1, R * S - 1, R * S, R * S + 1]


SCAN_VALUES = ("flags", "small", "large")


def scan_values(kind, n, rng):
    """0 / 1 flags; 0 .. 6; values up to floor((2^32 - 1) / n): the total stays below 2^32, a truncated partial sum shows."""
    if kind == "flags":
        return rng.integers(0, 2, size=n, dtype=np.uint64).astype(np.uint32)
    if kind == "small":
        return rng.integers(0, 7, size=n, dtype=np.uint64).astype(np.uint32)
    assert kind == "large"
    return rng.integers(0, (2 ** 32 - 1) // n + 1, size=n, dtype=np.uint64).astype(np.uint32)


def run_keys(n, S, shift):
    """n sorted 64-bit keys in runs of 1, 2, 64, 65 and S + 1, over and over; runs 2k and 2k + 1 differ below bit `shift` only."""
    lengths, total = [], 0
    while total < n:
        for m in (1, 2, 64, 65, S + 1):
            lengths.append(m)
            total += m
    run = np.repeat(np.arange(len(lengths), dtype=np.uint64), lengths)[:n]
    return ((run // np.uint64(2) + np.uint64(1 << 40)) << np.uint64(shift)) | (run % np.uint64(2))


# ---- the calls ------------------------------------------------------------------------------------------------------------
def _geometry(geo):
    return Geometry(*[int(x) for x in geo])


def _sort(hip, keys, vals, bits, begin_bit, check_from_bit=0, doc_off=None, expect=0):
    """(keys, vals, geometry) of the device's sort; the guards behind both are checked here."""
    n, guard = keys.size, hip.DEBUG_GUARD
    k = np.concatenate([keys, np.full(guard, 0x11111111, dtype=keys.dtype)])
    v = np.concatenate([vals.astype(np.uint32), np.full(guard, 0x11111111, dtype=np.uint32)])
    before = (k.copy(), v.copy())
    geo = np.zeros(9, dtype=np.uint32)
    off = None if doc_off is None else np.array(doc_off, dtype=np.int64)
    rc = hip.load().east_hip_debug_radix_sort_ex(0, keys.dtype.itemsize, k.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(_u32p), n,
                                                 bits, begin_bit, check_from_bit, None if off is None else off.ctypes.data_as(_i64p),
                                                 0 if off is None else off.size - 1, geo.ctypes.data_as(_u32p))
    assert rc == expect, (rc, hip.load().east_hip_last_error())
    if expect:
        assert np.array_equal(k, before[0]) and np.array_equal(v, before[1]) and not geo.any()
        return None
    assert (k[n:] == (EE64 if keys.dtype == np.uint64 else EE32)).all() and (v[n:] == EE32).all(), "a write behind the n pairs"
    return k[:n], v[:n], _geometry(geo)


def _check_sort(hip, keys, vals, bits, begin_bit, check_from_bit=0, doc_off=None, what=None):
    k, v, _ = _sort(hip, keys, vals, bits, begin_bit, check_from_bit, doc_off)
    rk, rv = sort_exact.sort_pairs(keys, vals, bits, begin_bit, doc_off)
    for name, got, want in (("keys", k, rk), ("vals", v, rv)):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, name, keys.size, bits, begin_bit, check_from_bit, "first differing positions", bad[:8], got[bad[:8]], want[bad[:8]])


def _scan(hip, form, a, expect=0):
    n, n_out = a.size, a.size + (1 if sort_exact.FORMS[form] == "with_total" else 0) if 0 <= form < len(sort_exact.FORMS) else a.size
    out = np.full(n_out + hip.DEBUG_GUARD, 0x11111111, dtype=np.uint32)
    geo = np.zeros(9, dtype=np.uint32)
    rc = hip.load().east_hip_debug_scan_ex(0, form, a.ctypes.data_as(_u32p), n, out.ctypes.data_as(_u32p), geo.ctypes.data_as(_u32p))
    assert rc == expect, (rc, hip.load().east_hip_last_error())
    if expect:
        assert (out == 0x11111111).all() and not geo.any()
        return None
    assert (out[n_out:] == EE32).all(), "a write behind the outputs"
    return out[:n_out], _geometry(geo)


@pytest.fixture(scope="module")
def geometry(hip):
    geo = _scan(hip, 0, np.ones(1, dtype=np.uint32))[1]
    assert geo.guard == hip.DEBUG_GUARD and geo.guard >= geo.tile and geo.guard >= geo.scan_tile
    assert geo.tile % 256 == 0 and geo.group >= 2 and geo.total_shards >= 2 and geo.spine_held_groups % geo.spine_parts == 0
    assert tuple(sort_exact.FORMS.index(f) for f in sort_exact.FORMS) == (hip.SCAN_EXCLUSIVE, hip.SCAN_INCLUSIVE, hip.SCAN_EXCLUSIVE_IN_PLACE,
                                                                         hip.SCAN_INCLUSIVE_IN_PLACE, hip.SCAN_WITH_TOTAL)
    return geo


# ---- radix sort, one segment ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,bits,begin_bit", bit_ranges(np.uint32) + bit_ranges(np.uint64))
def test_flat_sizes_and_bit_ranges(hip, geometry, dtype, bits, begin_bit):
    """Every size at every bit range: the bits outside [begin_bit, bits) come back with their pair and order nothing."""
    rng = np.random.default_rng(np.dtype(dtype).itemsize * 10000 + bits * 100 + begin_bit)
    for n in flat_sizes(geometry):
        keys = compose(random_field(n, bits - begin_bit, rng), dtype, bits, begin_bit, rng)
        _check_sort(hip, keys, np.arange(n, dtype=np.uint32), bits, begin_bit)


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_flat_values_are_carried(hip, geometry, dtype):
    """Values are carried, not interpreted: random ones, 0xFFFFFFFF and the guard's own pattern among them."""
    rng = np.random.default_rng(np.dtype(dtype).itemsize)
    for n in flat_sizes(geometry):
        keys = compose(random_field(n, 8, rng), dtype, 13, 5, rng)
        vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        vals[::3] = 0xFFFFFFFF
        vals[1::7] = EE32
        _check_sort(hip, keys, vals, 13, 5)


@pytest.mark.parametrize("distribution", DISTRIBUTIONS)
@pytest.mark.parametrize("dtype,bits,begin_bit", [(np.uint32, 8, 0), (np.uint32, 29, 5), (np.uint64, 8, 0), (np.uint64, 40, 8)])
def test_flat_distributions(hip, geometry, dtype, bits, begin_bit, distribution):
    """The digit streams a histogram, a packed wave counter or a ballot multisplit can get wrong, met by the first pass as they
    are, at every size from a tile on, with the one-bin test of the histogram on in every pass, off in the first, off in all:
    CHECK may only change speed."""
    rng = np.random.default_rng(DISTRIBUTIONS.index(distribution) * 100 + bits)
    T = geometry.tile
    for n in [m for m in flat_sizes(geometry) if m >= T - 1]:
        keys = make_keys(digit_stream(distribution, n, geometry, rng), dtype, bits, begin_bit, rng)
        vals = np.arange(n, dtype=np.uint32)
        for check_from_bit in (0, begin_bit + 8, bits + 8):
            _check_sort(hip, keys, vals, bits, begin_bit, check_from_bit, what=distribution)


# ---- radix sort, segmented ------------------------------------------------------------------------------------------------
def _doc_lists(geo):
    G = geo.group * geo.tile
    return {"6_documents": document_lengths(geo, 6), "11_documents": document_lengths(geo, 11), "300_small": small_document_lengths(),
            "one_document": [3 * G + 5]}


@pytest.mark.parametrize("distribution", ["equal", "uniform"])
@pytest.mark.parametrize("begin_bit", [0, 8])
@pytest.mark.parametrize("dtype,bits", [(np.uint32, 32), (np.uint64, 40)])
@pytest.mark.parametrize("docs", ["6_documents", "11_documents", "300_small", "one_document"])
def test_segmented(hip, geometry, docs, dtype, bits, begin_bit, distribution):
    """One call per document list, every document sorted in its own range: per-document tiles, virtual tiles, both spine
    kernels in the same pass (the lists of 6 and 11), a row of totals per shard (fewer documents than shards) and one row."""
    lengths = _doc_lists(geometry)[docs]
    doc_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(doc_off[-1])
    rng = np.random.default_rng(len(lengths) * 1000 + bits + begin_bit)
    width = bits - begin_bit
    field = np.full(n, (0x5A5A5A5A5A5A5A5A >> (64 - width)), dtype=np.uint64) if distribution == "equal" else random_field(n, width, rng)
    keys = compose(field, dtype, bits, begin_bit, rng)
    _check_sort(hip, keys, np.arange(n, dtype=np.uint32), bits, begin_bit, 0, doc_off, what=(docs, distribution))


# ---- the spine alone ------------------------------------------------------------------------------------------------------
def _spine(hip, group_sum, digit_total, doc_off=None, expect=0):
    guard = hip.DEBUG_GUARD
    group_sum, digit_total = np.ascontiguousarray(group_sum, dtype=np.uint32), np.ascontiguousarray(digit_total, dtype=np.uint32)
    prefix = np.full(group_sum.size + guard, 0x11111111, dtype=np.uint32)
    nxt = np.full(digit_total.size + guard, 0x11111111, dtype=np.uint32)
    geo = np.zeros(9, dtype=np.uint32)
    off = None if doc_off is None else np.array(doc_off, dtype=np.int64)
    rc = hip.load().east_hip_debug_radix_spine(0, group_sum.ctypes.data_as(_u32p), group_sum.shape[0], digit_total.ctypes.data_as(_u32p),
                                               None if off is None else off.ctypes.data_as(_i64p), 0 if off is None else off.size - 1,
                                               prefix.ctypes.data_as(_u32p), nxt.ctypes.data_as(_u32p), geo.ctypes.data_as(_u32p))
    assert rc == expect, (rc, hip.load().east_hip_last_error())
    if expect:
        assert (prefix == 0x11111111).all() and (nxt == 0x11111111).all() and not geo.any()
        return None
    assert (prefix[group_sum.size:] == EE32).all() and (nxt[digit_total.size:] == EE32).all(), "a write behind the outputs"
    return prefix[:group_sum.size].reshape(-1, 256), nxt[:digit_total.size]


def _check_spine(hip, group_sum, digit_total, doc_group0, doc_off, shards, what):
    prefix, nxt = _spine(hip, group_sum, digit_total, None if len(doc_off) == 1 else doc_off)
    want = sort_exact.spine(group_sum, digit_total, doc_group0, doc_off, shards)
    bad = np.argwhere(prefix != want)
    assert bad.size == 0, (what, "first differing (group, digit)", bad[:8].tolist(), [int(prefix[g, d]) for g, d in bad[:8]],
                           [int(want[g, d]) for g, d in bad[:8]])
    assert not nxt.any(), (what, "the other totals buffer is not cleared")


@pytest.mark.parametrize("kind", SPINE_KINDS)
def test_spine_flat(hip, geometry, kind):
    """One segment: the column-parallel kernel at every number of groups around its parts and around the switch from the
    stretch held in registers to the streamed one."""
    rng = np.random.default_rng(SPINE_KINDS.index(kind))
    G = geometry.group * geometry.tile
    for n_groups in spine_flat_groups(geometry):
        group_sum, total = spine_table(kind, n_groups, 1, geometry.total_shards, G, rng)
        _check_spine(hip, group_sum, total, [0, n_groups], [0], geometry.total_shards, (kind, n_groups))


@pytest.mark.parametrize("n_docs", [6, 9])
@pytest.mark.parametrize("kind", SPINE_KINDS)
def test_spine_segmented(hip, geometry, kind, n_docs):
    """Documents on both sides of the largest that radix_spine_docs_kernel takes, the column-parallel kernel for the others
    in the same step; a row of totals per shard (6 documents) and one row (9)."""
    rng = np.random.default_rng(10 + SPINE_KINDS.index(kind) + n_docs)
    G, big = geometry.group * geometry.tile, geometry.spine_doc_groups
    groups = [1, 2, big, big + 1, big + 2, 200] + [1, big + 1, big][:n_docs - 6]
    groups = [groups[k] for k in rng.permutation(n_docs)]
    lengths = [g * G - int(rng.integers(0, geometry.tile)) for g in groups]
    doc_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    doc_group0 = sort_exact.doc_groups(doc_off, geometry.tile, geometry.group)
    assert np.diff(doc_group0).tolist() == groups
    shards = geometry.total_shards if n_docs < geometry.total_shards else 1
    group_sum, total = spine_table(kind, doc_group0[-1], n_docs, shards, G, rng, doc_group0=doc_group0)
    _check_spine(hip, group_sum, total, doc_group0, doc_off, shards, (kind, groups))


# ---- the scans ------------------------------------------------------------------------------------------------------------
# (the sizes of the default geometry name the cases; the test takes them from the library's)
@pytest.mark.parametrize("size_index", range(14))
@pytest.mark.parametrize("form", sort_exact.FORMS)
def test_scan_forms(hip, geometry, form, size_index):
    """Every form at every size: with the total, n = S - 1, S and raw_tiles * S are where n + 1 crosses a tile and flips the
    raw path."""
    sizes = scan_sizes(geometry)
    assert len(sizes) == 14
    n = sizes[size_index]
    rng = np.random.default_rng(n)
    for kind in SCAN_VALUES:
        a = scan_values(kind, n, rng)
        got, _ = _scan(hip, sort_exact.FORMS.index(form), a)
        want = sort_exact.scan(a, form)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (form, n, kind, "first differing positions", bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("shift", [0, 12])
def test_run_heads(hip, geometry, shift):
    S, guard = geometry.scan_tile, hip.DEBUG_GUARD
    for n in (S - 1, S, S + 1, 3 * S + 7):
        keys = run_keys(n, S, 12)
        inc = np.full(n + guard, 0x11111111, dtype=np.uint32)
        count = np.full(1, 0x11111111, dtype=np.uint32)
        rc = hip.load().east_hip_debug_run_heads(0, keys.ctypes.data_as(_u64p), n, shift, inc.ctypes.data_as(_u32p), count.ctypes.data_as(_u32p))
        assert rc == 0, hip.load().east_hip_last_error()
        want, heads = sort_exact.run_heads(keys, shift)
        assert np.array_equal(inc[:n], want), (n, shift)
        assert (inc[n:] == EE32).all() and int(count[0]) == heads, (n, shift, int(count[0]), heads)


def _pair_bounded(hip, a, b, n_dev, extra, expect=0):
    n, guard = a.size, hip.DEBUG_GUARD
    out = [np.full(n + guard, 0x11111111, dtype=np.uint32) for _ in range(2)]
    rc = hip.load().east_hip_debug_scan_pair_bounded(0, a.ctypes.data_as(_u32p), b.ctypes.data_as(_u32p), n, n_dev, extra,
                                                     out[0].ctypes.data_as(_u32p), out[1].ctypes.data_as(_u32p))
    assert rc == expect, (rc, hip.load().east_hip_last_error())
    return out


@pytest.mark.parametrize("tiles,rest", [(1, 0), (3, 7)])
def test_scan_pair_bounded(hip, geometry, tiles, rest):
    """The bound is known on the device alone.  Both outputs equal the reference on [0, bound) and nothing is written at or
    behind n; nor is anything written in [bound, n) -- scan.h says so of its kernels (a store guard that tests n where it
    should test the bound changes nothing else)."""
    S = geometry.scan_tile
    n = tiles * S + rest
    rng = np.random.default_rng(n)
    a, b = scan_values("flags", n, rng), scan_values("large", n, rng)
    for k, target in enumerate([1, 2, 5, S - 1, S, S + 1, 2 * S + 3, n, n + 10]):
        extra = k % 2
        out_a, out_b = _pair_bounded(hip, a, b, target - extra, extra)
        bound, want_a, want_b = sort_exact.pair_bounded(a, b, target - extra, extra)
        assert bound == min(n, target)
        assert np.array_equal(out_a[:bound], want_a) and np.array_equal(out_b[:bound], want_b), (n, target)
        assert (out_a[n:] == EE32).all() and (out_b[n:] == EE32).all(), (n, target, "a write at or behind n")
        assert (out_a[bound:n] == EE32).all() and (out_b[bound:n] == EE32).all(), (n, target, "a write between the bound and n")


def _offsets(hip, values, n_values, expect=0):
    values = np.ascontiguousarray(values, dtype=np.uint32)
    off = np.full(n_values + 1 + hip.DEBUG_GUARD, 0x11111111, dtype=np.uint32)
    rc = hip.load().east_hip_debug_ascending_offsets(0, values.ctypes.data_as(_u32p), values.size, n_values, off.ctypes.data_as(_u32p))
    assert rc == expect, (rc, hip.load().east_hip_last_error())
    return off


def test_ascending_offsets(hip, geometry):
    S = geometry.scan_tile
    rng = np.random.default_rng(7)
    # values with none at the start (0 .. 4), in the middle (300 .. 599) and at the end (900 on), n_values above the largest
    pool = np.concatenate([np.arange(5, 300), np.arange(600, 900)])
    for values, n_values in ((np.array([3]), 7), (np.array([0]), 0), (np.sort(rng.choice(pool, size=S + 1)), 1000),
                             (np.sort(rng.choice(np.array([2, 3, 9]), size=S + 1)), 12)):
        off = _offsets(hip, values, n_values)
        assert np.array_equal(off[:n_values + 1], sort_exact.ascending_offsets(values, n_values)), (values.size, n_values)
        assert (off[n_values + 1:] == EE32).all()


# ---- what is turned away before any device work -----------------------------------------------------------------------------
def test_rejections(hip, geometry):
    """Null pointers, a bit range that is empty or wider than the key, a key width that is none, offsets that do not
    increase or do not end at n, more documents than the limit, an unknown scan form: EAST_HIP_ERR_INVALID, outputs untouched."""
    lib = hip.load()
    keys, vals = np.arange(10, dtype=np.uint32)[::-1].copy(), np.arange(10, dtype=np.uint32)
    _sort(hip, keys, vals, 8, 0)
    _sort(hip, keys, vals, 8, 0, doc_off=[0, 4, 10])
    for bits, begin_bit in ((8, 8), (8, 9), (0, 0), (33, 0), (8, -1)):
        _sort(hip, keys, vals, bits, begin_bit, expect=ERR_INVALID)
    _sort(hip, keys.astype(np.uint64), vals, 65, 0, expect=ERR_INVALID)
    _sort(hip, keys, vals, 8, 0, check_from_bit=-1, expect=ERR_INVALID)
    for doc_off in ([0, 4, 4, 10], [0, 5, 4, 10], [0, 4, 9], [0, 4, 11], [1, 4, 10], [0, 12, 10]):
        _sort(hip, keys, vals, 8, 0, doc_off=doc_off, expect=ERR_INVALID)
    _sort(hip, np.zeros(65536, dtype=np.uint32), np.zeros(65536, dtype=np.uint32), 8, 0, doc_off=np.arange(65537), expect=ERR_INVALID)
    geo = np.zeros(9, dtype=np.uint32)
    k, v = np.zeros(10 + hip.DEBUG_GUARD, dtype=np.uint32), np.zeros(10 + hip.DEBUG_GUARD, dtype=np.uint32)
    args = lambda kk, vv, gg, key_bytes=4: (0, key_bytes, None if kk is None else kk.ctypes.data_as(ctypes.c_void_p),
                                            None if vv is None else vv.ctypes.data_as(_u32p), 10, 8, 0, 0, None, 0,
                                            None if gg is None else gg.ctypes.data_as(_u32p))
    for bad in (args(None, v, geo), args(k, None, geo), args(k, v, None), args(k, v, geo, 2), args(k, v, geo, 16), args(k, v, geo, 0)):
        assert lib.east_hip_debug_radix_sort_ex(*bad) == ERR_INVALID
    off = np.array([0, 10], dtype=np.int64)
    assert lib.east_hip_debug_radix_sort_ex(0, 4, k.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(_u32p), 10, 8, 0, 0, None, 1,
                                            geo.ctypes.data_as(_u32p)) == ERR_INVALID
    assert lib.east_hip_debug_radix_sort_ex(0, 4, k.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(_u32p), 0, 8, 0, 0, off.ctypes.data_as(_i64p), 0,
                                            geo.ctypes.data_as(_u32p)) == ERR_INVALID
    assert not k.any() and not v.any() and not geo.any()
    # the spine: the number of groups must be the documents'
    G = geometry.group * geometry.tile
    gs, tot = np.ones((3, 256), dtype=np.uint32), np.ones((geometry.total_shards * 2, 256), dtype=np.uint32)
    _spine(hip, gs, tot, doc_off=[0, G, 3 * G])
    _spine(hip, gs, tot, doc_off=[0, G, 3 * G + 1], expect=ERR_INVALID)
    _spine(hip, gs, tot, doc_off=[0, 2 * G, 2 * G], expect=ERR_INVALID)
    _spine(hip, gs[:0], tot, expect=ERR_INVALID)
    # the scans
    a = np.arange(5, dtype=np.uint32)
    for form in (-1, len(sort_exact.FORMS), 99):
        _scan(hip, form, a, expect=ERR_INVALID)
    out = np.zeros(5 + 1 + hip.DEBUG_GUARD, dtype=np.uint32)
    p = lambda x: None if x is None else x.ctypes.data_as(_u32p)
    for bad in ((0, 0, None, 5, p(out), p(geo)), (0, 0, p(a), 5, None, p(geo)), (0, 0, p(a), 5, p(out), None), (0, 0, p(a), 0, p(out), p(geo)),
                (0, 0, p(a), -1, p(out), p(geo))):
        assert lib.east_hip_debug_scan_ex(*bad) == ERR_INVALID
    k64, count = np.arange(5, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
    for bad in ((0, None, 5, 0, p(out), p(count)), (0, k64.ctypes.data_as(_u64p), 5, 64, p(out), p(count)),
                (0, k64.ctypes.data_as(_u64p), 5, -1, p(out), p(count)), (0, k64.ctypes.data_as(_u64p), 5, 0, None, p(count)),
                (0, k64.ctypes.data_as(_u64p), 5, 0, p(out), None), (0, k64.ctypes.data_as(_u64p), 0, 0, p(out), p(count))):
        assert lib.east_hip_debug_run_heads(*bad) == ERR_INVALID
    for bad in ((0, None, p(a), 5, 1, 1, p(out), p(out)), (0, p(a), None, 5, 1, 1, p(out), p(out)), (0, p(a), p(a), 5, 1, 1, None, p(out)),
                (0, p(a), p(a), 5, 1, 1, p(out), None), (0, p(a), p(a), 0, 1, 1, p(out), p(out)), (0, p(a), p(a), 5, 0xFFFFFFFF, 1, p(out), p(out))):
        assert lib.east_hip_debug_scan_pair_bounded(*bad) == ERR_INVALID
    for bad in ((0, None, 5, 7, p(out)), (0, p(a), 5, 7, None), (0, p(a), 0, 7, p(out)), (0, p(a), 5, -1, p(out))):
        assert lib.east_hip_debug_ascending_offsets(*bad) == ERR_INVALID
    assert not out.any() and not count.any() and not geo.any()
