"""The five entry points that read device-resident hypothesis rows (gtnx_batch_ctc_score, _ctc_score_grad,
_ctc_token_align, _asg_score, _asg_score_grad): every rule the arguments alone decide, broken one at a time on a good
argument list, is GTNX_INVALID_ARGUMENT (1) with exactly the text written out here, with or without a device; a call
without pairs is OK and counts nothing.  The texts are the interface (callers match on them), so they are pinned as
whole strings, not as fragments."""
import ctypes

import pytest

p = ctypes.c_void_p

# what the three share, by the index in the argument list: 0 ems, 1 frames, 3 tokens, 4 row_stride, 5 lengths, 6 N, 7 L,
# 8 max_length (2 is blank for the CTC entries and the table for the ASG ones)
ROWS = [((0, None), "null batch handle"),  # (the C ABI's own text: it refuses the handle before the entry sees it)
        ((3, None), "null input pointer (tokens and lengths are both read)"),
        ((5, None), "null input pointer (tokens and lengths are both read)"),
        ((6, -1), "negative N or L"),
        ((7, -1), "negative N or L"),
        ((4, -1), "negative row stride"),
        ((4, 3), "row_stride is shorter than the rows' width L"),
        ((8, 0), "max_length outside 1 .. 4096"),
        ((8, 4097), "max_length outside 1 .. 4096"),
        ((8, -5), "max_length outside 1 .. 4096"),
        # (one element cannot overflow an int: TWO stands for the handle of a batch of two)
        ((0, "TWO", 6, 1 << 30), "n times N does not fit an int")]
BLANK = [((2, -1), "negative blank")]
TABLE = [((2, None), "null table pointer")]

#         name: (arguments after the handle, the entry's own rules, the *_stats getter)
ENTRIES = {
    "gtnx_batch_ctc_score": (
        #  1 frames 2 blank 3 tokens 4 stride 5 lengths 6 N 7 L 8 U 9 scores
        [None, 0, p(64), 4, p(64), 1, 4, 4, p(64)],
        ROWS + BLANK + [((9, None), "null scores pointer")], "debug_ctc_score_stats"),
    "gtnx_batch_ctc_score_grad": (
        #  ... 9 weights 10 grad
        [None, 0, p(64), 4, p(64), 1, 4, 4, p(64), p(64)],
        ROWS + BLANK + [((9, None), "null weights or grad pointer"), ((10, None), "null weights or grad pointer")],
        "debug_ctc_score_stats"),
    "gtnx_batch_ctc_token_align": (
        #  ... 9 scores 10 starts 11 ends 12 token scores 13 out_stride 14 frame tokens 15 frame_stride
        [None, 0, p(64), 4, p(64), 1, 4, 4, p(64), p(64), p(64), p(64), 4, p(64), 2],
        ROWS + BLANK + [((9, None), "null output pointer (scores, starts and ends are all written)"),
                        ((10, None), "null output pointer (scores, starts and ends are all written)"),
                        ((11, None), "null output pointer (scores, starts and ends are all written)"),
                        ((13, -1), "negative row stride"),
                        ((13, 3), "out_stride is shorter than the rows' width L"),
                        ((15, -1), "negative row stride")], "debug_ctc_token_align_stats"),
    "gtnx_batch_asg_score": (
        #  1 frames 2 table 3 tokens 4 stride 5 lengths 6 N 7 L 8 U 9 scores
        [None, p(64), p(64), 4, p(64), 1, 4, 4, p(64)],
        ROWS + TABLE + [((9, None), "null scores pointer")], "debug_asg_score_stats"),
    "gtnx_batch_asg_score_grad": (
        #  ... 9 weights 10 grad_emissions 11 grad_table
        [None, p(64), p(64), 4, p(64), 1, 4, 4, p(64), p(64), p(64)],
        ROWS + TABLE + [((9, None), "null weights pointer"),
                        ((10, None, 11, None), "neither gradient asked for (both pointers null)")],
        "debug_asg_score_stats"),
}
CASES = [(name, change, text) for name, (_, rules, _) in ENTRIES.items() for change, text in rules]


def changed(good, change):
    a = list(good)
    for i, v in zip(change[::2], change[1::2]):
        a[i] = v
    return a


@pytest.fixture
def batch(gtn):
    return gtn.Batch([gtn.linear_graph(2, 8)])


@pytest.fixture
def two(gtn):
    return gtn.Batch([gtn.linear_graph(2, 8), gtn.linear_graph(2, 8)])


@pytest.mark.parametrize("name,change,text", CASES, ids=[f"{n[11:]}-{'-'.join(map(str, c))}" for n, c, _ in CASES])
def test_one_broken_rule_gets_its_message(gtn, batch, two, name, change, text):
    import gtn_amd
    lib = gtn_amd._lib
    good = [batch._h] + ENTRIES[name][0]
    args = [two._h if v == "TWO" else v for v in changed(good, change)]
    assert getattr(lib, name)(*args) == 1
    want = text if text == "null batch handle" else f"[{name}] {text}"
    assert lib.gtnx_last_error().decode() == want


def test_every_rule_of_every_entry_is_covered():
    """the lists above, counted: the shared rules on all five, and each entry's own"""
    for name, (good, rules, _) in ENTRIES.items():
        texts = {t for _, t in rules}
        assert {t for _, t in ROWS} <= texts, name
        assert ("negative blank" in texts) == ("ctc" in name) and ("null table pointer" in texts) == ("asg" in name)
        assert all(i <= len(good) for c, _ in rules for i in c[::2]), name
    assert len(CASES) == 5 * len(ROWS) + 5 + 1 + 2 + 6 + 1 + 2


@pytest.mark.parametrize("name", ENTRIES)
def test_a_call_without_pairs_is_ok_and_counts_nothing(gtn, batch, name):
    """N == 0 (a batch without elements has no handle to give): OK without a device, nothing launched"""
    import gtn_amd
    stats = getattr(gtn, ENTRIES[name][2])
    before = stats()
    good = [batch._h] + ENTRIES[name][0]
    assert getattr(gtn_amd._lib, name)(*changed(good, (6, 0))) == 0
    if name == "gtnx_batch_asg_score_grad":  # (either gradient alone)
        assert getattr(gtn_amd._lib, name)(*changed(good, (6, 0, 10, None))) == 0
        assert getattr(gtn_amd._lib, name)(*changed(good, (6, 0, 11, None))) == 0
    assert stats() == before
