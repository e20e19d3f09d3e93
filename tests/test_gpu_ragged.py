"""GPU tests (-m gpu) of ragged batches: a count per channel through aggregate, the DEGA float entry, `encode csv` and the
LZMH chain, each through its entry point of the C ABI.  Everything is compared bit for bit (a NaN only has to be a NaN) with
tests/golden/ragged.npz: per channel what the compiled reference's chain gives on that channel's own count[c] readings.
No channel is left out.  Every row at or beyond a channel's count holds poison (NaN, +inf, 3e38, -0.0), in the fixture's
readings and in everything these tests build."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from agg_common import meter, same_floats  # noqa: E402
from ragged_common import CASES, FACTOR, HONEST, LEVELS, SETS, Fixture, poisoned, same_rows, same_streams, same_texts, untouched  # noqa: E402

pytestmark = pytest.mark.gpu

ORDER = [60, 1, 7]  # the caller's order is kept
INVALID = -1


@pytest.fixture(scope="module")
def dca():
    return load_package()


@pytest.fixture(scope="module")
def ctx(dca):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    c = dca.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return Fixture()


@pytest.fixture(params=["planned", "shared"])
def sharing(request, monkeypatch):
    """ "shared" lowers the planner's workgroup floor through its test knob so that the levels share a pass (the K = 3 form
    of the counted kernel); "planned" gives every level of these narrow batches a pass of its own (K = 1)"""
    if request.param == "shared":
        monkeypatch.setenv("DEGA_AGG_LEVELS_MIN_WORKGROUPS", "1")
    return request.param


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- aggregate ------------------------------------------------------------------------------------------------------------------

def test_aggregate_levels_counted(dca, ctx, fx, sharing):
    import torch
    for case in CASES:
        v, count = fx.v(case), fx.count(case)
        T, Cn = v.shape
        if sharing == "shared":
            assert len(dca.aggregate_levels_plan(Cn, T, ORDER)[1]) == 1
        outs = [torch.full((-(-T // N), Cn), -12345.0, dtype=torch.float32, device="cuda") for N in ORDER]
        sums, counts, err = ctx.aggregate_levels(dev(v), ORDER, out=outs, count=dev(count))  # 16-byte loads when C % 4 == 0
        assert (host(err) == 0).all()
        for k, N in enumerate(ORDER):
            g = host(sums[k])
            assert (host(counts[k]) == fx.rows(case, N)).all(), (case, N)
            assert same_rows(g, fx.sums(case, N), fx.rows(case, N)), (case, N)
            assert untouched(g, fx.rows(case, N), np.float32(-12345.0)), (case, N)  # a group without a reading is not stored
        # the same rows four bytes further on take the dword form; one level alone is K = 1
        flat = torch.zeros(T * Cn + 1, dtype=torch.float32, device="cuda")
        shifted = flat[1:].view(T, Cn)
        shifted.copy_(dev(v))
        assert shifted.data_ptr() % 16 != 0
        sums, counts, err = ctx.aggregate_levels(shifted, ORDER, count=dev(count))
        for k, N in enumerate(ORDER):
            assert (host(counts[k]) == fx.rows(case, N)).all() and same_rows(host(sums[k]), fx.sums(case, N), fx.rows(case, N)), (case, N, "dword")
        one, rows, err = ctx.aggregate(dev(v), 7, count=dev(count))
        assert (host(rows) == fx.rows(case, 7)).all() and same_rows(host(one), fx.sums(case, 7), fx.rows(case, 7)) and (host(err) == 0).all()


def test_aggregate_levels_counted_channels_and_pitches(ctx, fx):
    """channels= sub-ranges of a wider matrix, a pitch of its own per level: columns beyond are neither read into a result nor written"""
    import torch
    for case in CASES:
        v, count = fx.v(case), fx.count(case)
        T, Cn = v.shape
        for n in (Cn, Cn - 3, 64, 5):
            wide = torch.full((T, Cn + 4), float("inf"), dtype=torch.float32, device="cuda")
            wide[:, :Cn] = dev(v)
            outs = [torch.full((-(-T // N), n + (8, 1, 4)[k]), -12345.0, dtype=torch.float32, device="cuda") for k, N in enumerate(ORDER)]
            sums, counts, err = ctx.aggregate_levels(wide, ORDER, channels=n, out=outs, count=dev(count))
            assert (host(err) == 0).all() and err.numel() == n
            for k, N in enumerate(ORDER):
                g = host(sums[k])
                rows = fx.rows(case, N)[:n]
                assert (host(counts[k]) == rows).all() and same_rows(g[:, :n], fx.sums(case, N)[:, :n], rows), (case, n, N)
                assert (g[:, n:] == np.float32(-12345.0)).all() and untouched(g[:, :n], rows, np.float32(-12345.0)), (case, n, N)


def test_count_above_T_everywhere(ctx, fx):
    """count[c] > T: that channel gets ERROR_INVALID_VALUE, no output and counts of 0 from every entry point; its neighbours
    are what the fixture says"""
    case = "long"
    v, count = fx.v(case), fx.count(case).copy()
    T, Cn = v.shape
    bad = [3, 70, 131]
    count[bad] = [T + 1, 2 ** 40, 2 ** 62]
    keep = np.ones(Cn, dtype=bool)
    keep[bad] = False
    vd, cd = dev(v), dev(count)
    sums, counts, err = ctx.aggregate_levels(vd, ORDER, count=cd)
    e = host(err)
    assert (e[bad] == INVALID).all() and (e[keep] == 0).all()
    for k, N in enumerate(ORDER):
        rows = fx.rows(case, N).copy()
        rows[bad] = 0
        assert (host(counts[k]) == rows).all() and same_rows(host(sums[k]), fx.sums(case, N), rows), N
    text, lens, err = ctx.csv_write(vd, count=cd)
    want, want_len = fx.text(case, 1)
    t, n, e = host(text), host(lens), host(err)
    assert (e[bad] == INVALID).all() and (n[bad] == 0).all() and (e[keep] == 0).all()
    assert same_texts(t[keep], n[keep], want[keep], want_len[keep]) == ""
    for N, (out, bits, err, counts) in zip(ORDER, ctx.encode_f32_levels(vd, ORDER, FACTOR, 1, 32, count=cd)):
        o, b, e = host(out), host(bits), host(err)
        wo, wb, we = fx.dega(case, N, 32, 1)
        assert (e[bad] == INVALID).all() and (b[bad] == 0).all(), N
        assert same_streams(o[keep], b[keep], e[keep], wo[keep], wb[keep], we[keep]) == "", N
        assert (host(counts)[bad] == 0).all(), N
    for N, (out, bits, text_len, err, counts) in zip(ORDER, ctx.lzmh_encode_levels_f32(vd, ORDER, 2048, count=cd)):
        o, b, e = host(out), host(bits), host(err)
        wo, wb = fx.lzmh(case, N)
        assert (e[bad] == INVALID).all() and (b[bad] == 0).all() and (host(counts)[bad] == 0).all(), N
        assert same_streams(o[keep], b[keep], e[keep], wo[keep], wb[keep], np.zeros(Cn, dtype=np.int32)[keep]) == "", N


# ---- the DEGA float entry ----------------------------------------------------------------------------------------------------

def test_encode_f32_counted_all_sets(ctx, fx):
    for case in CASES:
        vd, cd = dev(fx.v(case)), dev(fx.count(case))
        for vs, ad in SETS:
            out, bits, err, counts = ctx.encode_f32(vd, FACTOR, ad, valuesize=vs, count=cd)
            assert same_streams(host(out), host(bits), host(err), *fx.dega(case, 1, vs, ad)) == "", (case, vs, ad)
            assert (host(counts) == fx.count(case)).all()
        # every level's (poisoned) sums with that level's counts, straight into the counted encoder
        for N in (7, 60):
            out, bits, err, _ = ctx.encode_f32(dev(fx.poisoned_sums(case, N)), FACTOR, 1, count=dev(fx.rows(case, N)))
            assert same_streams(host(out), host(bits), host(err), *fx.dega(case, N, 32, 1)) == "", (case, N)


def test_encode_f32_levels_counted(ctx, fx, sharing):
    for case in CASES:
        vd, cd = dev(fx.v(case)), dev(fx.count(case))
        for vs, ad in SETS:
            got = ctx.encode_f32_levels(vd, ORDER, FACTOR, ad, vs, count=cd)
            for N, (out, bits, err, counts) in zip(ORDER, got):
                assert same_streams(host(out), host(bits), host(err), *fx.dega(case, N, vs, ad)) == "", (case, N, vs, ad)
                assert (host(counts) == fx.rows(case, N)).all(), (case, N)
        out, bits, err, counts = ctx.encode_f32(vd, FACTOR, 1, num_values=7, count=cd)  # one level: the same call with K = 1
        assert same_streams(host(out), host(bits), host(err), *fx.dega(case, 7, 32, 1)) == "" and (host(counts) == fx.rows(case, 7)).all()


# ---- encode csv and the LZMH chain ---------------------------------------------------------------------------------------------

def test_csv_write_counted(ctx, fx, monkeypatch):
    for store in ("8", "64"):
        monkeypatch.setenv("DEGA_CSV_STORE", store)
        for case in CASES:
            for N in LEVELS:
                want, want_len = fx.text(case, N)
                rows = fx.rows(case, N)
                a = dev(fx.poisoned_sums(case, N))
                text, lens, err = ctx.csv_write(a, count=dev(rows))
                assert (host(err) == 0).all() and same_texts(host(text), host(lens), want, want_len) == "", (case, N, store)
                for n in (rows.size - 1, 33):  # channels= sub-ranges
                    text, lens, err = ctx.csv_write(a, channels=n, count=dev(rows))
                    assert text.shape[0] == n and (host(err) == 0).all() and same_texts(host(text), host(lens), want, want_len, channels=n) == "", (case, N, n)


def test_lzmh_encode_levels_counted(ctx, fx, sharing):
    for case in CASES:
        vd, cd = dev(fx.v(case)), dev(fx.count(case))
        Cn = vd.shape[1]
        for n in (Cn, 65):
            got = ctx.lzmh_encode_levels_f32(vd, ORDER, [1024, 2048, 1024], channels=n, count=cd)
            for N, (out, bits, text_len, err, counts) in zip(ORDER, got):
                want, want_bits = fx.lzmh(case, N)
                assert same_streams(host(out), host(bits), host(err), want, want_bits, np.zeros(Cn, dtype=np.int32), channels=n) == "", (case, N, n)
                assert (host(text_len) == fx.text(case, N)[1][:n]).all() and (host(counts) == fx.rows(case, N)[:n]).all(), (case, N, n)


# ---- round trips and the real chain --------------------------------------------------------------------------------------------

def test_round_trip_encode_decode_write(ctx, fx):
    """encode_f32(count) -> decode_f32 with counts -> csv_write(count) is the fixture's level-1 text"""
    for case in CASES:
        v, count = fx.v(case), fx.count(case)
        out, bits, err, counts = ctx.encode_f32(dev(v), FACTOR, 1, count=dev(count))
        back, got_count, derr = ctx.decode_f32(out, bits, v.shape[0], FACTOR, 1, var=True)
        assert (host(derr) == 0).all() and (host(got_count) == count).all(), case
        assert same_rows(host(back), v, count), case  # (two-decimal readings survive factor 100)
        text, lens, err = ctx.csv_write(back, count=got_count)
        assert (host(err) == 0).all() and same_texts(host(text), host(lens), *fx.text(case, 1)) == "", case


def test_round_trip_lzmh_levels(ctx, fx):
    """lzmh_encode_levels_f32(count) -> lzmh_decode_f32 returns the sums (what two decimals keep of them) and their counts"""
    for case in CASES:
        v, count = fx.v(case), fx.count(case)
        got = ctx.lzmh_encode_levels_f32(dev(v), ORDER, 2048, count=dev(count))
        for N, (out, bits, text_len, err, counts) in zip(ORDER, got):
            rows = fx.rows(case, N)
            back, got_count, back_len, derr = ctx.lzmh_decode_f32(out, bits, 2048, -(-v.shape[0] // N))
            # (a channel without a reading is the one case that does not come back: its stream has 0 bits, and the reference's
            # `decode lzmh` makes one 0x00 byte of an empty stream, which `decode csv` reads as one value, +0.0f)
            some = rows > 0
            assert (host(derr) == 0).all() and (host(got_count) == np.where(some, rows, 1)).all(), (case, N)
            assert (host(back_len)[some] == host(text_len)[some]).all() and (host(text_len)[~some] == 0).all(), (case, N)
            printed = np.array([[float("%.2f" % x) for x in row] for row in fx.sums(case, N)], dtype=np.float32)  # what two decimals keep of a sum
            assert same_rows(host(back), printed, rows), (case, N)


def test_the_real_chain_text_to_streams(ctx, fx, sharing):
    """csv_read of the fixture's base texts -- files of different line counts -- gives values and counts; those go straight into
    encode_f32_levels(count=) and lzmh_encode_levels_f32(count=); the results are the fixture's streams"""
    import torch
    for case in CASES:
        text, text_len = fx.text(case, 1)
        T, Cn = fx.v(case).shape
        stride = (text.shape[1] + 16 + 15) // 16 * 16
        padded = np.full((Cn, stride), 0x37, dtype=np.uint8)  # (bytes behind a text are not zeros)
        for c in range(Cn):
            padded[c, : int(text_len[c])] = text[c, : int(text_len[c])]
        values, count, err = ctx.csv_read(dev(padded), dev(text_len), T)
        assert (host(err) == 0).all() and (host(count) == fx.count(case)).all(), case
        assert same_rows(host(values), fx.v(case), fx.count(case)), case
        # what the reader leaves behind a channel's count is unspecified: make it poison
        values = torch.where(torch.arange(T, device="cuda")[:, None] < count[None, :], values, dev(poisoned(np.zeros((T, Cn), dtype=np.float32), fx.count(case))))
        for N, (out, bits, err, counts) in zip(ORDER, ctx.encode_f32_levels(values, ORDER, FACTOR, 1, 32, count=count)):
            assert same_streams(host(out), host(bits), host(err), *fx.dega(case, N, 32, 1)) == "", (case, N)
        for N, (out, bits, tl, err, counts) in zip(ORDER, ctx.lzmh_encode_levels_f32(values, ORDER, 2048, count=count)):
            assert same_streams(host(out), host(bits), host(err), *fx.lzmh(case, N), np.zeros(Cn, dtype=np.int32)) == "", (case, N)


def test_all_counts_equal_T_is_the_uniform_call(ctx):
    """one call with every count equal to T returns exactly the bytes of the uniform entry points"""
    import torch
    rng = np.random.default_rng(77)
    T, Cn = 203, 132
    v = meter(rng, T, Cn)
    v[5, 9] = -0.0
    vd = dev(v)
    cd = torch.full((Cn,), T, dtype=torch.int64, device="cuda")
    levels = [1, 7, 60]
    sums, counts, err = ctx.aggregate_levels(vd, levels, count=cd)
    for k, (a, b) in enumerate(zip(sums, ctx.aggregate_levels(vd, levels))):
        assert same_floats(host(a), host(b)) and (host(counts[k]) == -(-T // levels[k])).all()
    for vs, ad in SETS:
        one, uni = ctx.encode_f32(vd, FACTOR, ad, valuesize=vs, count=cd), ctx.encode_f32(vd, FACTOR, ad, valuesize=vs)
        assert all((host(a) == host(b)).all() for a, b in zip(one[:3], uni)), (vs, ad)
        for a, b in zip(ctx.encode_f32_levels(vd, levels, FACTOR, ad, vs, count=cd), ctx.encode_f32_levels(vd, levels, FACTOR, ad, vs)):
            assert all((host(x) == host(y)).all() for x, y in zip(a[:3], b)), (vs, ad)
    a, b = ctx.csv_write(vd, count=cd), ctx.csv_write(vd)
    assert (host(a[1]) == host(b[1])).all() and same_texts(host(a[0]), host(a[1]), host(b[0]), host(b[1])) == "" and (host(a[2]) == host(b[2])).all()
    for x, y in zip(ctx.lzmh_encode_levels_f32(vd, levels, 4096, count=cd), ctx.lzmh_encode_levels_f32(vd, levels, 4096)):
        assert all((host(p) == host(q)).all() for p, q in zip(x[:4], y))


def test_uniform_and_counted_calls_on_two_streams_share_the_scratches(ctx):
    """a uniform and a counted level call on one context, back to back on different streams without a synchronisation in
    between, in both orders: the two lay the sums block out differently (the counted call keeps per-channel statuses where
    the uniform call keeps its first level's sums), and every result equals that of the same call made alone"""
    import torch
    rng = np.random.default_rng(91)
    T, Cn, bad = 2000, 1024, 517
    va, vb = dev(meter(rng, T, Cn, top=30.0)), dev(meter(rng, T, Cn, top=3000.0))
    count = rng.integers(0, T + 1, Cn).astype(np.int64)
    count[bad] = T + 1
    cb = dev(count)
    levels = [1, 7]
    stride = T * 9 + 16
    pairs = {
        "dega": (lambda: ctx.encode_f32_levels(va, levels), lambda: ctx.encode_f32_levels(vb, levels, count=cb), 2),
        "lzmh": (lambda: ctx.lzmh_encode_levels_f32(va, levels, stride), lambda: ctx.lzmh_encode_levels_f32(vb, levels, stride, count=cb), 3),
    }

    def same(got, want):  # per level (out, bits, ..., err[, counts]): the streams as far as the longest goes, the rest in full
        for g, w in zip(got, want):
            nbytes = (int(w[1].max()) + 7) // 8
            if not (len(g) == len(w) and torch.equal(g[0][:, :nbytes], w[0][:, :nbytes]) and all(torch.equal(x, y) for x, y in zip(g[1:], w[1:]))):
                return False
        return len(got) == len(want)

    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for name, (uniform, counted, status) in pairs.items():
        alone = []
        for call in (uniform, counted):
            res = call()
            torch.cuda.synchronize()
            alone.append([[t.clone() for t in level] for level in res])
        for lu, lc in zip(*alone):
            assert not torch.equal(lu[1], lc[1]), name  # (a mix-up of the two batches would show)
            assert (lu[status] == 0).all(), name
            assert int(lc[status][bad]) == INVALID and int(lc[1][bad]) == 0, name
        for first, second in ((0, 1), (1, 0)):
            torch.cuda.synchronize()
            with torch.cuda.stream(s1):
                r1 = (uniform, counted)[first]()
            with torch.cuda.stream(s2):
                r2 = (uniform, counted)[second]()
            torch.cuda.synchronize()
            assert same(r1, alone[first]) and same(r2, alone[second]), (name, first)


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(dca, ctx):
    import torch
    L = dca.library()
    E = dca.ERROR_INVALID_VALUE
    s = ctx._stream()
    T, Cn = 64, 8
    v = dev(meter(np.random.default_rng(1), T, Cn))
    count = torch.full((Cn + 1,), T, dtype=torch.int64, device="cuda")
    sums = torch.full((2, T, Cn), -12345.0, dtype=torch.float32, device="cuda")
    rows = torch.full((2, Cn + 1), 77, dtype=torch.int64, device="cuda")
    err = torch.full((2, Cn), 77, dtype=torch.int32, device="cuda")
    out = torch.full((2, Cn, 2048), 0xEE, dtype=torch.uint8, device="cuda")
    bits = torch.full((2, Cn), 77, dtype=torch.int64, device="cuda")
    lens = torch.full((2, Cn), 77, dtype=torch.int64, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    arr = lambda xs, t=C.c_void_p: (t * max(1, len(xs)))(*xs)  # noqa: E731
    two = lambda t: arr((p(t[0]), p(t[1])))  # noqa: E731
    nv = arr((2, 4), C.c_size_t)
    ld2 = arr((Cn, Cn), C.c_size_t)
    caps = arr((2048, 2048), C.c_size_t)

    def agg(cnt=p(count), oc=None, er=p(err), nvs=nv, K=2, ld=Cn):
        return L.dega_hip_aggregate_levels_var_dev(ctx._h, p(v), Cn, T, ld, cnt, nvs, K, two(sums), ld2, two(rows) if oc is None else oc, er, s)

    misaligned_rows = arr((p(rows[0]), p(rows[1]) + 4))
    assert agg(cnt=None) == E and agg(cnt=p(count) + 4) == E  # a null count, a misaligned one
    assert agg(oc=misaligned_rows) == E and agg(oc=arr((p(rows[0]), None))) == E and agg(er=None) == E and agg(er=p(err) + 2) == E
    assert agg(nvs=arr((2, 0), C.c_size_t)) == E and agg(nvs=arr((4, 4), C.c_size_t)) == E and agg(ld=Cn - 1) == E  # the uniform twin's refusals
    assert L.dega_hip_aggregate_levels_var_dev(ctx._h, p(v), Cn, 2 ** 32, Cn, p(count), nv, 2, two(sums), ld2, two(rows), p(err), s) == E

    def enc(cnt=p(count), vs=32, cap=2048, ld=Cn, T_=T):
        return L.dega_hip_encode_f32_var_dev(ctx._h, p(v), Cn, T_, ld, cnt, 100.0, 1, vs, p(out[0]), cap, p(bits[0]), p(err[0]), s)

    assert enc(cnt=None) == E and enc(cnt=p(count) + 4) == E and enc(vs=0) == E and enc(vs=65) == E and enc(cap=2046) == E and enc(ld=Cn - 1) == E
    assert enc(T_=2 ** 25 + 1) == E

    def lev(cnt=p(count), oc=None, nvs=nv, cps=caps):
        return L.dega_hip_encode_levels_f32_var_dev(ctx._h, p(v), Cn, T, Cn, cnt, nvs, 2, 100.0, 1, 32, two(out), cps, two(bits), two(rows) if oc is None else oc,
                                                    two(err), s)

    assert lev(cnt=None) == E and lev(cnt=p(count) + 4) == E and lev(oc=misaligned_rows) == E and lev(nvs=arr((2, 2), C.c_size_t)) == E
    assert lev(cps=arr((2048, 2046), C.c_size_t)) == E
    assert L.dega_hip_encode_levels_f32_var_dev(ctx._h, p(v), Cn, T, Cn, p(count), nv, 2, 100.0, 1, 32, two(out), caps, two(bits), None, two(err), s) == E  # out_count is required

    text = out[0]

    def csv(cnt=p(count), d=2, stride=2048, o=None, ld=Cn):
        return L.dega_hip_csv_write_var_dev(ctx._h, p(v), Cn, T, ld, cnt, d, 1, 44, p(text) if o is None else o, stride, p(lens[0]), p(err[0]), s)

    assert csv(cnt=None) == E and csv(cnt=p(count) + 4) == E and csv(d=7) == E and csv(stride=2040) == E and csv(o=p(text) + 8) == E and csv(ld=Cn - 1) == E

    def lz(cnt=p(count), oc=None, ts=(2048, 2048), cps=caps):
        return L.dega_hip_lzmh_encode_levels_f32_var_dev(ctx._h, p(v), Cn, T, Cn, cnt, nv, 2, 2, 1, 44, arr(ts, C.c_size_t), two(out), cps, two(bits), two(lens),
                                                         two(rows) if oc is None else oc, two(err), s)

    assert lz(cnt=None) == E and lz(cnt=p(count) + 4) == E and lz(oc=misaligned_rows) == E and lz(ts=(2048, 1000)) == E and lz(cps=arr((2048, 32), C.c_size_t)) == E
    assert L.dega_hip_lzmh_encode_levels_f32_var_dev(ctx._h, p(v), Cn, T, Cn, p(count), nv, 2, 2, 1, 44, arr((2048, 2048), C.c_size_t), two(out), caps, two(bits),
                                                     two(lens), None, two(err), s) == E
    torch.cuda.synchronize()
    for t, fill in ((sums, -12345.0), (rows, 77), (err, 77), (out, 0xEE), (bits, 77), (lens, 77)):
        assert (t == fill).all()  # nothing was launched
    # K = 0 and C = 0: nothing to do
    assert L.dega_hip_aggregate_levels_var_dev(ctx._h, p(v), Cn, T, Cn, p(count), None, 0, None, None, None, p(err), s) == 0
    assert L.dega_hip_encode_f32_var_dev(ctx._h, p(v), 0, T, Cn, None, 100.0, 1, 32, p(out[0]), 2048, p(bits[0]), p(err[0]), s) == 0
    assert L.dega_hip_csv_write_var_dev(ctx._h, p(v), 0, T, Cn, None, 2, 1, 44, p(text), 2048, p(lens[0]), p(err[0]), s) == 0
    torch.cuda.synchronize()
    assert (err == 77).all() and (rows == 77).all()
    # T = 0 still launches: counts of 0 are fine, anything above is above T
    count0 = torch.zeros(Cn, dtype=torch.int64, device="cuda")
    count0[2] = 1
    assert L.dega_hip_aggregate_levels_var_dev(ctx._h, None, Cn, 0, Cn, p(count0), nv, 2, two(sums), ld2, two(rows), p(err), s) == 0
    assert L.dega_hip_csv_write_var_dev(ctx._h, None, Cn, 0, Cn, p(count0), 2, 1, 44, p(text), 2048, p(lens[0]), p(err[1]), s) == 0
    torch.cuda.synchronize()
    want = [0, 0, INVALID, 0, 0, 0, 0, 0]
    assert host(err[0]).tolist() == want and host(err[1]).tolist() == want and (rows[:, :Cn] == 0).all() and (lens[0] == 0).all() and (sums == -12345.0).all()
