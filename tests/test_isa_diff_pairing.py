"""tools/isa_diff.py pairs the kernels of two builds by symbol and, where a symbol is gone, by content (no compiler, no GPU): hand-made
symbol -> disassembly lines and symbol -> descriptor dictionaries through pair_renamed."""
from tools.isa_diff import pair_renamed

A = ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_add_f64 v[0:1], v[2:3], v[4:5]", "s_endpgm"]
B = ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_mul_f64 v[0:1], v[2:3], v[4:5]", "s_endpgm"]
D = {"vgpr_count": "24", "agpr_count": "0", "sgpr_count": "16", "private_segment_fixed_size": "0"}


def test_a_clean_rename_is_paired_and_a_kept_symbol_is_left_to_the_symbol_comparison():
    old = {"k_keep": list(A), "k<OldArgs>": list(B)}
    new = {"k_keep": list(B), "k<NewArgs>": list(B)}                # k_keep differs, but it has its symbol on both sides: not this function's
    desc = lambda names: {n: dict(D) for n in names}               # noqa: E731
    assert pair_renamed(old, new, desc(old), desc(new)) == ({"k<OldArgs>": "k<NewArgs>"}, [], [])


def test_one_changed_instruction_or_one_changed_descriptor_entry_is_no_rename():
    old, new = {"k<OldArgs>": list(A)}, {"k<NewArgs>": A[:1] + ["v_add_f64 v[0:1], v[2:3], v[6:7]"] + A[2:]}
    assert pair_renamed(old, new, {"k<OldArgs>": dict(D)}, {"k<NewArgs>": dict(D)}) == ({}, ["k<OldArgs>"], ["k<NewArgs>"])
    new = {"k<NewArgs>": list(A)}                                   # the same instructions with one more register
    assert pair_renamed(old, new, {"k<OldArgs>": dict(D)}, {"k<NewArgs>": dict(D, vgpr_count="25")}) == ({}, ["k<OldArgs>"], ["k<NewArgs>"])
    assert pair_renamed(old, new, {"k<OldArgs>": dict(D)}, {"k<NewArgs>": dict(D)}) == ({"k<OldArgs>": "k<NewArgs>"}, [], [])


def test_two_identical_candidates_for_one_kernel_pair_nothing():
    old = {"k<OldArgs>": list(A), "other": list(B)}
    new = {"k<New, false>": list(A), "k<New, true>": list(A), "other": list(B)}
    desc = lambda names: {n: dict(D) for n in names}               # noqa: E731
    assert pair_renamed(old, new, desc(old), desc(new)) == ({}, ["k<OldArgs>"], ["k<New, false>", "k<New, true>"])
    # the mirror image: two identical old kernels and one candidate
    assert pair_renamed(new, old, desc(new), desc(old)) == ({}, ["k<New, false>", "k<New, true>"], ["k<OldArgs>"])


def test_twins_on_both_sides_pair_in_symbol_order():
    """two instantiations that compile to the same code, renamed together: every one has a partner of equal content"""
    old = {"k<false, Old>": list(A), "k<true, Old>": list(A), "j<Old>": list(B)}
    new = {"k<true, New>": list(A), "k<false, New>": list(A), "j<New>": list(B)}
    desc = lambda names: {n: dict(D) for n in names}               # noqa: E731
    assert pair_renamed(old, new, desc(old), desc(new)) == ({"j<Old>": "j<New>", "k<false, Old>": "k<false, New>", "k<true, Old>": "k<true, New>"}, [], [])


def test_a_kernel_missing_on_one_side_stays_unpaired():
    old = {"k<OldArgs>": list(A), "gone": list(B)}
    new = {"k<NewArgs>": list(A)}
    desc = lambda names: {n: dict(D) for n in names}               # noqa: E731
    assert pair_renamed(old, new, desc(old), desc(new)) == ({"k<OldArgs>": "k<NewArgs>"}, ["gone"], [])
    assert pair_renamed(new, old, desc(new), desc(old)) == ({"k<NewArgs>": "k<OldArgs>"}, [], ["gone"])
    assert pair_renamed({}, {"added": list(A)}, {}, {"added": dict(D)}) == ({}, [], ["added"])
