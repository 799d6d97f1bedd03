"""CPU: the arithmetic of tests/many_frames.py — where the 2^31 and 2^32 byte crossings of each case's buffers fall, that the
seven-image pattern tells the frames at every crossing apart, and the whole-call limit the cases stay inside."""
import types

import numpy as np
import pytest

import many_frames as mf

G31, G32 = 1 << 31, 1 << 32


def test_largest_max_batch_is_the_documented_limit():
    assert mf.largest_max_batch(136, 200, "f32") == 2467 and mf.largest_max_batch(136, 200, "bf16") == 4934
    assert mf.largest_max_batch(2160, 3840, "f32") == 8 and mf.largest_max_batch(2160, 3840, "bf16") == 16
    assert mf.largest_max_batch(480, 752, "f32") == 185 and mf.largest_max_batch(480, 752, "bf16") == 371
    assert mf.largest_max_batch(16, 16, "f32") == mf.largest_max_batch(16, 16, "bf16") == 65535
    for H, W in ((136, 200), (2160, 3840), (480, 752), (72, 104)):
        for prec, R in mf.ROW_BYTES.items():
            b = mf.largest_max_batch(H, W, prec)
            assert b * mf.cells(H, W) * R < G31 <= (b + 1) * mf.cells(H, W) * R


def test_record_layout_of_the_cases():
    r = mf.record_layout(100, 136, 200)
    assert (r["hdr"], r["xy"], r["resp"], r["cov"], r["cinv"], r["desc"]) == (0, 16, 832, 1248, 2064, 2880)
    assert (r["occ"], r["dd"], r["sd"], r["bytes"]) == (106304, 107168, 108880, 110592)
    assert mf.record_layout(8, 16, 24)["bytes"] == 9728


# case -> {buffer: [(crossing, frame that holds it)]}: the buffers that reach a crossing at all
EXPECTED = {
    "act0_past_2_32": {"act0": [(G31, 308), (G32, 616)]},
    "max_grid_y": {"act0": [(G31, 21845), (G32, 43690)]},
    "halves_unequal": {"act0": [(G31, 308), (G32, 616)]},
    "act1_past_2_31": {"act0": [(G31, 616), (G32, 1233)], "act1": [(G31, 2467)]},
    "edge_f32": {"act0": [(G31, 308), (G32, 616)], "act1": [(G31, 1233)]},
    "edge_bf16": {"act0": [(G31, 616), (G32, 1233)], "act1": [(G31, 2467)]},
}


@pytest.mark.parametrize("name", list(mf.CASES))
@pytest.mark.parametrize("rot", [0, 3])
def test_crossings_and_pattern(name, rot):
    cs = mf.case(name)
    got, frames = mf.check_case(cs, rot)
    sizes = mf.frame_bytes(cs["H"], cs["W"], cs["nf"], cs["precision"])
    for buf, S in sizes.items():
        want = [(x, f) for x, f in EXPECTED[name].get(buf, []) if f < cs["B"]]
        if buf == "head":   # (the limit itself: the head activations of the largest call end just below 2^31)
            assert cs["B"] * S < G31 and got[buf] == []
            continue
        assert got[buf] == want, (name, buf, got[buf], want)
        for x, f in got[buf]:
            assert f * S < x < (f + 1) * S
            assert mf.image_of(f - 1, rot) != mf.image_of(f, rot) != mf.image_of(f + 1, rot) != mf.image_of(f - 1, rot)
            assert {f - 1, f} <= set(frames) and (f + 1 >= cs["B"] or f + 1 in frames)
    assert frames[0] == 0 and frames[-1] == cs["B"] - 1


def test_the_cases_reach_what_they_are_named_for():
    c = mf.case("act0_past_2_32")
    assert c["B"] * mf.frame_bytes(136, 200, 100, "f32")["act0"] == 4317184000 > G32 and c["B"] * mf.cells(136, 200) == 263500
    c = mf.case("max_grid_y")
    assert c["B"] == mf.GRID_Y_MAX and c["B"] * mf.cells(16, 24) == 393210
    c = mf.case("halves_unequal")
    assert (c["B"] // 2, c["B"] - c["B"] // 2) == (310, 311) and c["async_cov"]
    assert mf.crossings(c["B"], mf.frame_bytes(136, 200, 100, "f32")["act0"])[0][1] < 310   # inside the first half
    c = mf.case("act1_past_2_31")
    assert c["B"] * mf.frame_bytes(136, 200, 100, "bf16")["act1"] == 2149888000 > G31 and c["B"] * mf.cells(136, 200) == 1049750
    assert mf.case("edge_f32")["B"] == 2467 and mf.case("edge_bf16")["B"] == 4934
    assert mf.case("edge_f32")["B"] * mf.cells(136, 200) < 1 << 20 and mf.case("edge_bf16")["B"] * mf.cells(136, 200) < 1 << 21


def test_a_pattern_of_equal_neighbours_or_a_dividing_frame_is_caught():
    cs = dict(mf.case("act0_past_2_32"), H=128, W=256)   # 128 x 256 x 64 x 4 bytes divides 2^31
    with pytest.raises(AssertionError):
        mf.check_case(cs)
    cs = dict(mf.case("edge_f32"), B=2468)               # one frame beyond the limit
    with pytest.raises(AssertionError):
        mf.check_case(cs)


def test_the_record_comparison_names_the_frame_and_field_that_differ():
    """mismatches() on made-up records: a swapped image, one flipped bit in a row below K, and bytes behind K that do not count."""
    nf, H, W, n = 3, 16, 24, 40
    lay = mf.record_layout(nf, H, W)
    L = types.SimpleNamespace(bytes=lay["bytes"], off_hdr=lay["hdr"], off_xy=lay["xy"], off_resp=lay["resp"], off_cov=lay["cov"],
                              off_cinv=lay["cinv"], off_desc=lay["desc"], off_occ=lay["occ"], off_dd=lay["dd"], off_sd=lay["sd"])
    rng = np.random.default_rng(5)
    c = mf.cells(H, W)
    refs = []
    for j in range(mf.K_IMAGES):
        k = 1 + j % 3
        f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
        refs.append(dict(K=k, n_candidates=k + j, kp_xy=f(k, 2), response=f(k), cov2=f(k, 2), cov2_inv=f(k, 2), desc=f(k, 256),
                         occ_grid=rng.integers(-1, k, (H // 8, W // 8)).astype(np.int16), dense_dust=f(c), semi_dust=f(c)))
    fields = [mf.reference_fields(L, r) for r in refs]

    def records(rot):
        recs = rng.integers(0, 256, (n, lay["bytes"]), dtype=np.uint8)   # (whatever lies behind row K and in the padding)
        for i in range(n):
            for _name, off, want in fields[mf.image_of(i, rot)]:
                recs[i, off:off + len(want)] = want
        return recs
    for rot in (0, 3, 5):
        assert mf.mismatches(records(rot), fields, rot) == []
        assert len(mf.mismatches(records(rot), fields, (rot + 1) % mf.K_IMAGES)) == 8      # (the limit of the report)
    recs = records(3)
    recs[17] = recs[18]                                   # frame 17 carries its neighbour's record
    recs[33, lay["desc"] + 1024 * (refs[mf.image_of(33, 3)]["K"] - 1) + 700] ^= 1       # one bit in the last row below K
    recs[5, lay["desc"] + 1024 * refs[mf.image_of(5, 3)]["K"]] ^= 1                     # behind row K: not compared
    bad = mf.mismatches(recs, fields, 3, limit=64)
    assert {b.split(":")[0] for b in bad} == {"frame 17 (image %d)" % mf.image_of(17, 3), "frame 33 (image %d)" % mf.image_of(33, 3)}
    assert "frame 33 (image %d): desc" % mf.image_of(33, 3) in bad and len([b for b in bad if b.startswith("frame 33")]) == 1
