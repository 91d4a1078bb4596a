"""CPU: the structured attention inputs and the per-element comparison of tests/attention_ref.py do what they claim -- the operands are exact
in bf16, the selector inputs select, the matches sit on every loop boundary, every planted fault is refused by at least 10 x the tolerance at
every sequence length, and the older criterion (max-norm on uniform random inputs) accepts such faults.  No GPU, a few seconds in total."""
import pytest
import torch

import attention_ref as ar

ALL_KINDS = ar.SELECTOR_KINDS + ar.OFFSET_KINDS


def _cases(kinds, shapes=ar.SHAPES):
    for B, T, H in shapes:
        for kind in kinds:
            yield ar.make_case(kind, B, T, H)


def test_every_operand_round_trips_through_bf16():
    for cs in _cases(ALL_KINDS):
        assert torch.equal(cs.op.double(), cs.built), (cs.kind, cs.T)                 # q' | k | v as built in float64
        assert cs.op.shape == (ar.pad_rows(cs.B * cs.T), 3 * cs.inner) and cs.dout.shape == (cs.op.shape[0], cs.inner)
        for t in (cs.op[:, 2 * cs.inner:], cs.dout, cs.out_pad):
            assert torch.equal(t.double(), t.double().round()) and t.double().abs().max() <= 4
        if cs.rows > cs.B * cs.T:                                                     # the padding rows are filled, not zero
            assert bool((cs.op[cs.B * cs.T:].double().abs().sum(-1) > 0).all()) and bool((cs.dout[cs.B * cs.T:].double().abs().sum(-1) > 0).all())
        assert not bool((cs.op.double() == ar.SENTINEL).any()) and not bool((cs.dout.double() == ar.SENTINEL).any())


def test_offset_scores_are_exact_in_fp32_and_sit_where_they_should():
    assert [ar.late_edge(T) for T in (96, 97, 128, 129, 289)] == [96, 96, 96, 128, 128]
    for cs in _cases(ar.OFFSET_KINDS, [(2, 97, 2), (2, 129, 2), (2, 289, 2)]):
        q, k, _ = cs.qkv(cs.op.double())                                              # the pre-scaled q': scores in log2 units
        s2 = q @ k.transpose(-1, -2)
        assert torch.equal(s2.float().double(), s2) and torch.equal(s2 * 64, (s2 * 64).round())
        centre = {"off-300": -300.0, "off+300": 300.0, "off+3008": 3008.0}.get(cs.kind)
        if centre is not None:
            assert (s2 - centre).abs().max() <= 56
        elif cs.kind == "mixed":                                                      # -300 / 0 / +300 interleaved inside every 32-query wave
            for r in range(3):
                assert (s2[:, :, r::3] - (-300.0, 0.0, 300.0)[r]).abs().max() <= 56
        else:                                                                         # "late": the first key tile 600 log2 units below the others
            e = ar.late_edge(cs.T)
            assert (s2[..., :e] + 300).abs().max() <= 56 and (s2[..., e:] - 300).abs().max() <= 56 and e < cs.T
            if cs.T > 128:                                                            # ... of the 96-key AND the 128-key form: a jump of at
                assert e >= 128                                                       # least 488 between tiles, exp2 of it is 0 in fp32
                assert s2[..., e:].min().item() - s2[..., :e].max().item() >= 488


def test_book_correlation_is_within_the_cap(monkeypatch):
    for seed in (0, 1, 2):
        for n in (129, 289, 393):
            c = ar.book(n, seed)
            corr = c @ c.T
            corr.fill_diagonal_(0)
            assert corr.abs().max().item() <= ar.BOOK_CAP and bool((c.abs() == 1).all())
    monkeypatch.setattr(ar, "BOOK_CAP", 16)                                             # a book over the cap is refused, not used
    with pytest.raises(ValueError):
        ar.book(129, 0)


def test_selector_probabilities_are_one_over_the_group_and_nothing_else():
    for cs in _cases(ar.SELECTOR_KINDS):
        q, k, v = cs.qkv()
        P = ar.attend(q, k, v, cs.d_o())["P"]
        assert P[~cs.match].numel() == 0 or P[~cs.match].max().item() < 2.0 ** -30, (cs.kind, cs.T)
        want = (1.0 / cs.size.double())[..., None].expand_as(P)
        assert (P[cs.match] - want[cs.match]).abs().max().item() <= 1e-12
        assert bool((cs.match.sum(-1) == cs.size).all())
        s2 = (q @ k.transpose(-1, -2)) * ar.ATTN_C                                    # log2 units: matched 128, every other one >= 40 below
        assert s2[cs.match].min().item() - (s2[~cs.match].max().item() if (~cs.match).any() else -1e9) >= 40
        sizes = set(cs.size.unique().tolist())
        assert sizes <= {1, 2, 4} and (cs.T < 4 or {"sel1": 1, "sel2": 2, "sel4": 4, "pm": 2}[cs.kind] in sizes)
        if cs.kind == "pm" and cs.T >= 2:                                             # unequal keys at equal score: dq has a value
            assert ar.attend(q, k, v, cs.d_o())["dq"].abs().max().item() > 1.0
        elif cs.kind != "pm":
            assert ar.attend(q, k, v, cs.d_o())["dq"].abs().max().item() < 1e-9


def test_matches_cover_every_loop_boundary():
    assert ar.boundaries(1) == [0] and ar.boundaries(33) == [0, 31, 32]
    assert ar.boundaries(129) == [0, 31, 32, 63, 64, 95, 96, 127, 128]
    assert set(ar.boundaries(289)) >= {0, 95, 96, 127, 128, 191, 192, 255, 256, 287, 288}
    for T in ar.T_LIST:
        bd = set(ar.boundaries(T))
        for tile in ar.TILES:                                                         # first and last row of every tile of every size, clipped to T
            assert {e for e in range(0, T, tile)} | {min(e + tile, T) - 1 for e in range(0, T, tile)} <= bd
        assert {0, T - 1} <= bd
    for cs in _cases(ar.SELECTOR_KINDS):
        q, k, v = cs.qkv()
        hit = ar.attend(q, k, v, cs.d_o())["P"] > 0.2                                 # read from the reference, not from the construction
        bd = ar.boundaries(cs.T)
        assert bool(hit[:, :, bd].any(-1).all()), "a boundary query without a matched key"
        assert bool(hit[:, :, :, bd].any(-2).all()), "a boundary key no query selects"
        assert bool(hit.any(-1).all()) and bool(hit.any(-2).all())
        if cs.T > 1:                                                                  # the permutations differ between every two (b, h)
            flat = hit.reshape(cs.B * cs.H, -1)
            assert all(not torch.equal(flat[a], flat[b]) for a in range(len(flat)) for b in range(a))


def test_written_out_gradients_equal_autograd():
    for cs in _cases(("pm", "sel4", "off+300", "late"), [(2, 97, 2), (2, 1, 2)]):
        q, k, v = cs.qkv()
        mine, auto = ar.attend(q, k, v, cs.d_o()), ar.autograd_reference(cs)
        for name in ("O", "lse", "delta", "dq", "dk", "dv"):
            assert (mine[name] - auto[name]).abs().max().item() <= 1e-9 * max(1.0, auto[name].abs().max().item()), (cs.kind, name)


def test_comparison_accepts_the_reference_and_refuses_non_finite_results():
    want = torch.tensor([0.0, 1.0, -4.0], dtype=torch.float64)
    assert ar.ratio(want, want, 2, 2.0 ** -9) == 0.0
    assert ar.ratio(want + torch.tensor([2.0 ** -9, 0, 0]), want, 2, 2.0 ** -9) == 1.0
    assert ar.ratio(want[1:] * (1 + 2.0 ** -8), want[1:], 2, 0.0) <= 1.0 < ar.ratio(want[1:] * (1 + 2.0 ** -7), want[1:], 2, 0.0)
    for bad in (float("nan"), float("inf"), float("-inf")):
        got = want.clone()
        got[1] = bad
        assert ar.ratio(got, want, 2, 1.0) == float("inf") and ar.ratio32(got, want, 128.0, 3) == float("inf")
        assert ar.ratio_lse(got, want, 3) == float("inf")
    assert abs(ar.ulp32(3008.0) - 2.0 ** -12) == 0 and ar.ulp32(1.0) == 2.0 ** -23


@pytest.mark.parametrize("T", ar.T_LIST)
def test_planted_faults_are_refused_by_ten_tolerances(T):
    """Every fault of ar.FAULTS on every selector input, B = 2, H = 2.  One (fault, T) pair is no fault at all and is asserted to be none: with
    T = 1 every (b, h) holds the one code of a one-code book, so head h+1's K block IS head h's."""
    for kind in ar.SELECTOR_KINDS:
        cs = ar.make_case(kind, 2, T, 2)
        q, k, v = cs.qkv()
        want = ar.attend(q, k, v, cs.d_o())
        for fault in ar.FAULTS:
            if fault == "head_K" and T == 1:
                assert torch.equal(k.roll(-1, 1), k)
                continue
            per = ar.rejections(cs, want, ar.planted(cs, fault))
            rej = max(per.values())
            assert rej >= 10.0, f"T={T} {kind} {fault}: refused by {rej:.2f} x the tolerance only"
            # The two passes of the backward read delta and mask their rows separately, so a pass that alone goes wrong must be refused
            # through its own outputs: a delta one row off through dq alone and through dk alone (not only through the delta output), rows
            # past T through dk alone and through dv alone.  (A leaked query that gives ALL its weight to one key has dS = P (dP - delta) = 0
            # whatever its dO: groups of one -- sel1, and T = 1 -- cannot show it in dk, and that is asserted to be so.)
            if fault == "rows_past_T_in_dkdv" and (kind == "sel1" or T == 1):
                assert per["dk"] < 1e-9 and per["dv"] >= 10.0
                continue
            for name in {"delta_next_row": ("dq", "dk"), "rows_past_T_in_dkdv": ("dk", "dv")}.get(fault, ()):
                assert per[name] >= 10.0, f"T={T} {kind} {fault}: refused through {name} by {per[name]:.2f} x the tolerance only"


@pytest.mark.parametrize("T", ar.T_LIST)
def test_forward_faults_are_refused_on_the_offset_inputs_too(T):
    """The offset floors are coarser than the selector ones (dk above all), so they are held against faults as well: every fault that reaches
    the forward is refused by at least 10 x the tolerance through O or lse alone, in every offset family."""
    for kind in ar.OFFSET_KINDS:
        cs = ar.make_case(kind, 2, T, 2)
        q, k, v = cs.qkv()
        want = ar.attend(q, k, v, cs.d_o())
        for fault in ("key_T_admitted", "key_T-1_dropped", "head_K", "head_V", "batch_rows", "v_chunks_swapped"):
            per = ar.rejections(cs, want, ar.planted(cs, fault))
            rej = max(per["O"], per["lse"])
            if kind == "late" and fault == "key_T_admitted" and T > ar.late_edge(T):   # the admitted key is the next sample's row 0, a LOW
                assert rej < 1e-9                                                     # key 488 log2 units under the row's high ones: it
                continue                                                              # carries no weight, "late" cannot show this fault
            assert rej >= 10.0, f"T={T} {kind} {fault}: refused by {rej:.2f} x the tolerance only"


def test_floors_are_four_times_the_measured_error_and_a_tenth_of_a_fault_at_most():
    """FLOORS is MEASURED times 4, nothing else; and on the selector inputs, where every fault is planted, every fault at every T moves
    some output by at least ten times that output's floor."""
    assert ar.FLOOR_FACTOR == 4 and set(ar.FLOORS) == set(ar.MEASURED) == set(ar.FAMILIES)
    for table, measured in ((ar.FLOORS, ar.MEASURED), (ar.FLOOR_F32, ar.MEASURED_F32)):
        for fam, per in measured.items():
            assert set(per) >= set(table[fam]) and all(m > 0 and table[fam][name] == 4 * m for name, m in per.items())
    for fam in ("off", "off3008"):                                                    # the coarse family lends nothing to the finer one
        assert all(ar.FLOORS["sel"][n] <= ar.FLOORS[fam][n] for n in ar.R)
    assert ar.FLOORS["off"]["dk"] <= ar.FLOORS["off3008"]["dk"] / 8                   # (|q| 52 against 521)
    worst_floor = {}
    for T in ar.T_LIST:                                                               # the element that refuses a fault is off by at least
        for kind in ar.SELECTOR_KINDS:                                                # 10 x (r 2^-9 |want| + floor) >= 10 x floor: held here
            cs = ar.make_case(kind, 2, T, 2)                                          # directly, fault by fault, on the output that shows it
            q, k, v = cs.qkv()
            want = ar.attend(q, k, v, cs.d_o())
            for fault in ar.FAULTS:
                bad = ar.planted(cs, fault)
                if fault == "head_K" and T == 1:
                    continue
                err = {n: (val - want[n]).abs().nan_to_num(float("inf")).max().item() for n, val in bad.items() if n in ar.R}
                assert any(ar.FLOORS["sel"][n] <= e / 10 for n, e in err.items()), (T, kind, fault, err)
                n = max(err, key=err.get)
                worst_floor[n] = max(worst_floor.get(n, 0.0), ar.FLOORS["sel"][n] / err[n])
    print("floor / error of the output a planted fault shows most in, largest over the faults:", {n: f"{x:.2g}" for n, x in worst_floor.items()})


def test_a_maximum_that_starts_at_zero_and_is_never_lowered_is_refused():
    for B, T, H in ((2, 33, 2), (2, 129, 2)):
        cs = ar.make_case("off-300", B, T, H)
        bad = ar.m_never_lowered(cs)
        assert bool((bad["l"] == 0).all())                                            # every P underflowed
        want = ar.autograd_reference(cs)
        assert ar.ratio(bad["O"], want["O"], ar.R["O"], ar.floors(cs.kind)["O"]) == float("inf")
        assert ar.ratio_lse(bad["lse"], want["lse"], T) == float("inf")
        zero = ar.m_never_lowered(ar.make_case("mixed", B, T, H))                     # (rows at offset 0 survive the shortcut: only far rows see it)
        assert bool(torch.isfinite(zero["O"][:, :, 1::3]).all()) and not bool(torch.isfinite(zero["O"][:, :, 0::3]).any())


def test_old_criterion_accepts_planted_faults_on_random_inputs():
    """Why this file exists: on the uniform random inputs of test_attention_fwd / test_attention_bwd at T = 1033 the max-norm bounds
    (1.5e-2 max|O|, 2e-3 on lse, 2.5e-2 max|dv|) ACCEPT two 16-byte chunks of a V row swapped in the forward (O within the bound, lse
    untouched) and one V chunk misplaced in the backward (dv within the bound): both asserted.  A key admitted past the sequence passes
    the bound on O (asserted) but the lse bound does catch it on some rows, and the 119 query rows of the next sample added to dk / dv
    the old bound does see: those figures are only printed."""
    cs = ar.random_case(2, 1033, 2)
    q, k, v = cs.qkv()
    want = ar.attend(q, k, v, cs.d_o())
    bad = ar.planted(cs, "key_T_admitted")                                            # O lets it through; lse's 2e-3 holds it on the worst rows only
    o_err, lse_err = (bad["O"] - want["O"]).abs().max().item(), (bad["lse"] - want["lse"]).abs()
    print(f"key T admitted, random inputs: O err {o_err:.2e}, lse err max {lse_err.max().item():.2e}, rows over 2e-3: {int((lse_err > 2e-3).sum())} of {lse_err.numel()}")
    assert 0 < o_err < 1.5e-2 * max(1.0, want["O"].abs().max().item())
    bad = ar.planted(cs, "v_chunks_swapped")
    assert 0 < (bad["O"] - want["O"]).abs().max().item() < 1.5e-2 * max(1.0, want["O"].abs().max().item())
    assert (bad["lse"] - want["lse"]).abs().max().item() == 0
    bad = ar.planted(cs, "rows_past_T_in_dkdv")
    for name in ("dk", "dv"):                                                         # (119 of 1033 rows too many: 2.5e-2 max|.| does see this one)
        err = (bad[name] - want[name]).abs().max().item()
        print(f"rows past T in {name}, random inputs: err {err:.2e} of max {want[name].abs().max().item():.2e}")
    vv = v.clone()                                                                    # one 16-byte chunk of one V row from its neighbour, in the backward
    vv[0, 1, 500, 16:24] = v[0, 1, 500, 24:32]
    bad = ar.attend(q, k, vv, cs.d_o())
    for name in ("dq", "dk", "dv"):
        err = (bad[name] - want[name]).abs().max().item()
        print(f"one V chunk misplaced, {name}, random inputs: err {err:.2e} of max {want[name].abs().max().item():.2e}")
    assert (bad["dv"] - want["dv"]).abs().max().item() <= 2.5e-2 * want["dv"].abs().max().item()
