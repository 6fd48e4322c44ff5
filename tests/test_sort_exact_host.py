"""CPU tier: pin the witness of tests/test_gpu_sort_scan_forms.py (tests/sort_exact.py) to brute-force restatements --
`sorted` with an explicit (document, masked key, index) key, running sums in a loop -- on inputs of a few hundred elements,
the segment and bit-range corners included; and the gpu file's case generators to what they were written to contain.
"""
import numpy as np
import pytest

import sort_exact
import test_gpu_sort_scan_forms as gpu_file

DEFAULT_GEOMETRY = gpu_file.Geometry(4096, 8, 8, 64, 2048, 4096, 2048, 4096, 32)    # csrc/radix_sort.h, csrc/scan.h as committed


def _brute_sort(keys, vals, bits, begin_bit, doc_off):
    ks, vs = [int(k) for k in keys], [int(v) for v in vals]
    mask = (1 << (bits - begin_bit)) - 1
    doc_of = [0] * len(ks)
    for d in range(len(doc_off) - 1):
        for i in range(doc_off[d], doc_off[d + 1]):
            doc_of[i] = d
    order = sorted(range(len(ks)), key=lambda i: (doc_of[i], (ks[i] >> begin_bit) & mask, i))
    return [ks[i] for i in order], [vs[i] for i in order]


@pytest.mark.parametrize("dtype,bits,begin_bit", [(np.uint32, 1, 0), (np.uint32, 8, 0), (np.uint32, 9, 0), (np.uint32, 13, 5),
                                                  (np.uint32, 17, 16), (np.uint32, 32, 24), (np.uint32, 32, 31), (np.uint32, 32, 0),
                                                  (np.uint64, 40, 8), (np.uint64, 64, 56), (np.uint64, 64, 0), (np.uint64, 64, 63)])
def test_sort_pairs(dtype, bits, begin_bit):
    rng = np.random.default_rng(bits * 64 + begin_bit)
    for n, doc_off in ((1, None), (2, [0, 1, 2]), (300, None), (300, [0, 300]), (300, [0, 1, 2, 65, 66, 299, 300]),
                       (257, [0, 256, 257])):
        # few values in the ordering bits (ties: stability), anything in the others
        width = bits - begin_bit
        few = rng.integers(0, 1 << min(width, 3), size=n, dtype=np.uint64) << np.uint64(begin_bit + max(0, width - 3))
        noise = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
        inside = np.uint64(((1 << width) - 1) << begin_bit)
        keys = ((noise & ~inside) | few).astype(dtype)
        vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        k, v = sort_exact.sort_pairs(keys, vals, bits, begin_bit, doc_off)
        bk, bv = _brute_sort(keys, vals, bits, begin_bit, [0, n] if doc_off is None else doc_off)
        assert k.dtype == dtype and [int(x) for x in k] == bk and [int(x) for x in v] == bv, (n, doc_off)
        assert np.array_equal(sort_exact.digits(keys, bits, begin_bit) << np.uint64(begin_bit), keys.astype(np.uint64) & inside)


def _brute_spine(group_sum, digit_total, doc_group0, doc_off, shards):
    out = [[0] * 256 for _ in range(len(group_sum))]
    for d in range(len(doc_group0) - 1):
        smaller = int(doc_off[d])
        for digit in range(256):
            run = smaller
            for g in range(doc_group0[d], doc_group0[d + 1]):
                out[g][digit] = run & 0xFFFFFFFF
                run += int(group_sum[g][digit])
            for k in range(shards):
                smaller += int(digit_total[d * shards + k][digit])
    return out


@pytest.mark.parametrize("doc_group0,shards", [([0, 1], 8), ([0, 7], 8), ([0, 1, 2, 5, 6], 8), ([0, 3, 4, 9], 1), ([0, 2, 3], 2)])
def test_spine(doc_group0, shards):
    rng = np.random.default_rng(len(doc_group0) + shards)
    n_docs, n_groups = len(doc_group0) - 1, doc_group0[-1]
    group_sum = rng.integers(0, 1 << 20, size=(n_groups, 256), dtype=np.uint32)
    group_sum[:, 7] = 0                                 # (a digit absent)
    digit_total = rng.integers(0, 1 << 24, size=(n_docs * shards, 256), dtype=np.uint32)        # (the spine does not ask that they agree)
    doc_off = np.concatenate([[0], np.cumsum(rng.integers(1, 1 << 28, size=n_docs))])[:n_docs]
    doc_off[-1] = 0xFFFFFF00 if n_docs > 1 else 0       # (sums that pass 2^32 wrap as the device's do)
    got = sort_exact.spine(group_sum, digit_total, doc_group0, doc_off, shards)
    assert got.dtype == np.uint32 and got.tolist() == _brute_spine(group_sum, digit_total, doc_group0, doc_off, shards)


def test_doc_groups():
    assert sort_exact.doc_groups([0, 1, 9, 9 + 32, 9 + 32 + 33, 200], 4, 8) == [0, 1, 2, 3, 5, 9]


@pytest.mark.parametrize("n", [1, 2, 5, 300])
def test_scans(n):
    rng = np.random.default_rng(n)
    for a in (rng.integers(0, 2, size=n), rng.integers(0, 7, size=n), rng.integers(0, (1 << 32) // n, size=n),
              np.full(n, 0xFFFFFFFF)):                  # (the last: sums that pass 2^32 wrap)
        a = a.astype(np.uint32)
        inc, run = [], 0
        for x in a.tolist():
            run += x
            inc.append(run & 0xFFFFFFFF)
        exc = [0] + inc[:-1]
        for form in sort_exact.FORMS:
            want = inc if form.startswith("inclusive") else exc + [inc[-1]] if form == "with_total" else exc
            got = sort_exact.scan(a, form)
            assert got.dtype == np.uint32 and got.tolist() == want, form


def test_run_heads():
    rng = np.random.default_rng(1)
    for shift in (0, 3, 40, 63):
        keys = np.sort(rng.integers(0, 1 << 62, size=200, dtype=np.uint64) >> np.uint64(rng.integers(0, 60)))
        keys = np.sort(np.concatenate([keys, keys[::3], keys[:5]]))
        inc, run = [], 0
        ks = [int(k) for k in keys]
        for i, k in enumerate(ks):
            run += 1 if i == 0 or (k >> shift) != (ks[i - 1] >> shift) else 0
            inc.append(run)
        got, count = sort_exact.run_heads(keys, shift)
        assert got.tolist() == inc and count == run and count == len(set(k >> shift for k in ks))
    assert sort_exact.run_heads(np.array([5], dtype=np.uint64), 0)[1] == 1


def test_pair_bounded():
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 9, size=100).astype(np.uint32), rng.integers(0, 1 << 20, size=100).astype(np.uint32)
    for n_dev, extra, want in ((0, 1, 1), (4, 1, 5), (99, 0, 99), (99, 1, 100), (100, 10, 100)):
        bound, ea, eb = sort_exact.pair_bounded(a, b, n_dev, extra)
        assert bound == want and ea.size == bound and eb.size == bound
        for got, src in ((ea, a), (eb, b)):
            run = 0
            for i in range(bound):
                assert got[i] == run
                run += int(src[i])


def test_ascending_offsets():
    for values, n_values in (([0], 0), ([3], 5), ([2, 2, 2, 5, 5, 9], 12), ([0, 0, 1, 4, 4, 4, 7], 7), ([1, 2, 3], 3)):
        want = [next((i for i, x in enumerate(values) if x >= v), len(values)) for v in range(n_values + 1)]
        got = sort_exact.ascending_offsets(np.array(values, dtype=np.uint32), n_values)
        assert got.dtype == np.uint32 and got.tolist() == want
        for v in range(n_values):
            assert values[want[v]:want[v + 1]] == [x for x in values if x == v]


# ---- the gpu file's generators at the default geometry: what each was written to contain ----------------------------------
def test_radix_sizes_and_distributions():
    geo = DEFAULT_GEOMETRY
    T, G = geo.tile, geo.group * geo.tile
    sizes = gpu_file.flat_sizes(geo)
    assert sizes == [1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 7 * T, 8 * T, 9 * T, 9 * T + 1, G - 1, G, G + 1, 8 * G + 1, 17 * T + 3]
    assert max(sizes) < 5500000
    n = 2 * G + 5
    for name in gpu_file.DISTRIBUTIONS:
        d = gpu_file.digit_stream(name, n, geo, np.random.default_rng(0))
        assert d.shape == (n,) and d.dtype == np.uint64 and int(d.max()) < 256, name
    d = lambda name: gpu_file.digit_stream(name, n, geo, np.random.default_rng(0)).tolist()
    assert len(set(d("equal"))) == 1
    assert d("ascending") == sorted(d("ascending")) and len(set(d("ascending"))) == 256
    assert d("descending") == sorted(d("descending"), reverse=True) and len(set(d("descending"))) == 256
    assert d("mod256")[:300] == [i % 256 for i in range(300)]
    r = d("runs64")
    assert all(len(set(r[i:i + 64])) == 1 for i in range(0, n - 64, 64)) and r[63] != r[64]
    r = d("runs64_shifted")
    assert all(len(set(r[i:i + 64])) == 1 for i in range(1, n - 64, 64)) and r[0] != r[1] and r[64] != r[65]
    r = d("all_but_one")
    assert sorted(np.bincount(r).tolist())[-2:] == [1, n - 1]
    r = d("switch_at_tile_and_group")
    assert [i for i in range(1, n) if r[i] != r[i - 1]] == [T, G]
    r = d("alternating")
    assert len(set(r)) == 2 and all(r[i] != r[i + 1] for i in range(n - 1))
    assert len(set(d("uniform"))) == 256


def test_keys_hold_the_digits_and_noise_outside():
    rng = np.random.default_rng(3)
    for dtype, bits, begin_bit in gpu_file.bit_ranges(np.uint32) + gpu_file.bit_ranges(np.uint64):
        dtype = np.dtype(dtype)
        stream = rng.integers(0, 256, size=500, dtype=np.uint64)
        keys = gpu_file.make_keys(stream, dtype, bits, begin_bit, np.random.default_rng(4))
        assert keys.dtype == dtype
        # the first pass's digit is the stream's (its low bits where the range is narrower than a digit) ...
        width = bits - begin_bit
        low = np.uint64((1 << min(width, 8)) - 1)
        assert np.array_equal(sort_exact.digits(keys, bits, begin_bit) & low, stream & low), (bits, begin_bit)
        # ... and the bits outside the range are not all alike where there are any
        outside = keys.astype(np.uint64) & ~np.uint64(((1 << width) - 1) << begin_bit)
        if width < dtype.itemsize * 8:
            assert np.unique(outside).size > 1, (bits, begin_bit)


def test_document_lists():
    geo = DEFAULT_GEOMETRY
    T, G, big = geo.tile, geo.group * geo.tile, geo.spine_doc_groups
    for n_docs in (6, 11):
        lengths = gpu_file.document_lengths(geo, n_docs)
        assert len(lengths) == n_docs and sum(lengths) < 5500000
        want = [1, 2, 63, T - 1, T, T + 1, G, G + 1, 3 * G + 5, big * G, big * G + 1]
        assert set(lengths) <= set(want) and {big * G, big * G + 1} <= set(lengths)
        if n_docs >= len(want):
            assert sorted(lengths) == sorted(want)
        off = np.concatenate([[0], np.cumsum(lengths)])
        assert any(o % 4 for o in off[1:-1])            # (offsets that are not 16-byte aligned)
        groups = np.diff(sort_exact.doc_groups(off, T, geo.group))
        assert groups.max() == big + 1 and sorted(groups)[-2] == big
    small = gpu_file.small_document_lengths()
    assert len(small) == 300 and set(small) == {1, 2, 3}


def test_spine_tables():
    geo = DEFAULT_GEOMETRY
    G = geo.group * geo.tile
    assert gpu_file.spine_flat_groups(geo) == [1, 31, 32, 33, 2047, 2048, 2049, 2050, 5000]
    for kind in gpu_file.SPINE_KINDS:
        gs, tot = gpu_file.spine_table(kind, 40, 1, geo.total_shards, G, np.random.default_rng(5))
        assert gs.shape == (40, 256) and tot.shape == (geo.total_shards, 256)
        assert (gs.sum(axis=1) == G).all() and np.array_equal(tot.sum(axis=0), gs.sum(axis=0))
        assert (tot > 0).sum(axis=0).max() > 1          # (more than one shard row holds something)
    gs, _ = gpu_file.spine_table("one_digit", 40, 1, 8, G, np.random.default_rng(5))
    assert ((gs > 0).sum(axis=1) == 1).all()
    gs, _ = gpu_file.spine_table("digit_absent", 40, 1, 8, G, np.random.default_rng(5))
    assert gs[:, 17].sum() == 0 and (gs.sum(axis=0) > 0).sum() > 200
    # segmented: the totals of a document are its own groups'
    g0 = [0, 3, 40]
    gs, tot = gpu_file.spine_table("multinomial", 40, 2, 8, G, np.random.default_rng(5), doc_group0=g0)
    for d in range(2):
        assert np.array_equal(tot[d * 8:(d + 1) * 8].sum(axis=0), gs[g0[d]:g0[d + 1]].sum(axis=0))


def test_scan_sizes_and_values():
    geo = DEFAULT_GEOMETRY
    S, R = geo.scan_tile, geo.scan_raw_tiles
    assert gpu_file.scan_sizes(geo) == [1, 3, 4, 5, 1023, 1024, 1025, S - 1, S, S + 1, 2 * S + 1, R * S - 1, R * S, R * S + 1]
    for n in (1, 5, 3 * S + 1):
        for kind in gpu_file.SCAN_VALUES:
            a = gpu_file.scan_values(kind, n, np.random.default_rng(6))
            assert a.dtype == np.uint32 and a.size == n and int(a.astype(np.uint64).sum()) < 1 << 32, kind
        if n > S:
            assert int(gpu_file.scan_values("large", n, np.random.default_rng(6)).astype(np.uint64).sum()) > 1 << 30
    keys = gpu_file.run_keys(S + 1, S, 12)
    assert keys.dtype == np.uint64 and keys.size == S + 1 and np.array_equal(keys, np.sort(keys))
    keys = gpu_file.run_keys(3 * S, S, 12)
    runs = np.diff(np.flatnonzero(np.concatenate([[1], keys[1:] != keys[:-1], [1]])))
    assert {1, 2, 64, 65, S + 1} <= set(runs.tolist())
    assert sort_exact.run_heads(keys, 12)[1] < sort_exact.run_heads(keys, 0)[1]         # (the shift merges neighbouring runs)
