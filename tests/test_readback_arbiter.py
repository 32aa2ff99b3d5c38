"""The packed-or-float choice of BFS's level read-back (graphlily_amd/readback.py) driven with synthetic durations: no GPU.
The expected sequences are what the driver's inline bookkeeping chose before it became this class (P = packed, F = float)."""
import collections

from graphlily_amd.readback import BookKey, ReadbackBook


def drive(book, calls, packed_s, float_s, pin="1"):
    """`calls` driver calls: choose, run that way for its synthetic time, record.  -> the ways as a string"""
    out = []
    for _ in range(calls):
        as_bytes = book.choose(True, False, pin)
        book.record("packed" if as_bytes else "float", packed_s if as_bytes else float_s)
        out.append("P" if as_bytes else "F")
    return "".join(out)


def test_packed_faster_float_tried_at_call_8_and_every_32nd():
    assert drive(ReadbackBook(), 70, 1.0, 2.0) == "PPPPPPPPFFFPPPPPPPPPPPPPPPPPPPPFPPPPPPPPPPPPPPPPPPPPPPPPPPPPPPPFPPPPPP"


def test_float_faster_packed_tried_every_32nd():
    assert drive(ReadbackBook(), 70, 2.0, 1.0) == "PPPPPPPPFFFFFFFFFFFFFFFFFFFFFFFPFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFPFFFFFF"


def test_pin_2_is_always_packed():
    assert drive(ReadbackBook(), 70, 2.0, 1.0, pin="2") == "P" * 70
    assert drive(ReadbackBook(), 70, 1.0, 2.0, pin="2") == "P" * 70


def test_packed_wins_ties():
    assert drive(ReadbackBook(), 70, 1.0, 1.0) == "PPPPPPPPFFFPPPPPPPPPPPPPPPPPPPPFPPPPPPPPPPPPPPPPPPPPPPPPPPPPPPPFPPPPPP"


def test_cannot_pack_is_float_and_leaves_the_books_alone():
    book = ReadbackBook()
    drive(book, 20, 1.0, 2.0)
    before = (book.calls, book.packed, book.float)
    for pin in ("0", "1", "2"):
        for timed in (False, True):
            assert book.choose(False, timed, pin) is False
    assert (book.calls, book.packed, book.float) == before
    fresh = ReadbackBook()
    assert fresh.choose(False, False, "1") is False and fresh.calls == 0


def test_timed_call_takes_can_pack_and_records_nothing():
    book = ReadbackBook()
    drive(book, 40, 2.0, 1.0)                    # float is the measured choice by now
    assert book.choose(True, False, "1") is False
    before = (book.calls, book.packed, book.float, book.report("float"))
    assert book.choose(True, True, "1") is True
    assert book.choose(False, True, "1") is False
    assert (book.calls, book.packed, book.float, book.report("float")) == before


def test_first_two_calls_of_a_way_are_not_recorded():
    book = ReadbackBook()
    book.record("packed", 12.0)
    book.record("packed", 12.0)
    assert book.packed is None and book.calls == 2
    book.record("packed", 1.0)
    assert book.packed == 1.0 and book.float is None and book.calls == 3
    book.record("float", 9.0)
    book.record("float", 9.0)
    assert book.float is None
    book.record("float", 3.0)
    assert book.float == 3.0 and book.calls == 6


def test_median_is_over_the_last_seven_samples():
    book = ReadbackBook()
    for _ in range(2 + 7):
        book.record("packed", 5.0)
    assert book.packed == 5.0
    for k in range(7):
        book.record("packed", 0.25)
        assert book.packed == (5.0 if k < 3 else 0.25)      # (the median turns over with the fourth fast sample of seven)
    assert book.packed == 0.25 and book.report("packed")["packed_ms"] == 250.0
    book.record("packed", 0.75)                  # (six of 0.25 and one of 0.75)
    assert book.packed == 0.25


def test_two_book_keys_do_not_share_state():
    books = collections.defaultdict(ReadbackBook)      # (what the driver keeps in bits_loop_["readback"])
    pull_push = BookKey(9, 0.001, 1.0, False, 0, 1 << 20)
    pull = BookKey(9, -1.0, 0.0, True, 0, 1 << 20)
    assert books[pull_push] is books[BookKey(9, 0.001, 1.0, False, 0, 1 << 20)]
    assert books[pull_push] is not books[pull]
    assert drive(books[pull_push], 40, 2.0, 1.0)[-1] == "F"
    assert books[pull].calls == 0 and books[pull].packed is None and books[pull].float is None
    assert drive(books[pull], 40, 1.0, 2.0)[-1] == "P"
    assert books[pull_push].choose(True, False, "1") is False and books[pull].choose(True, False, "1") is True
    assert books[BookKey(9, 0.001, 1.0, False, 64, 1 << 19)].calls == 0      # (another slice of the same schedule)


def test_report_is_none_until_measured_then_ms_to_four_decimals():
    book = ReadbackBook()
    assert book.report("packed") == {"way": "packed", "packed_ms": None, "float_ms": None}
    book.record("packed", 1.0)
    book.record("packed", 1.0)
    assert book.report("packed") == {"way": "packed", "packed_ms": None, "float_ms": None}
    book.record("packed", 0.00038912345)
    assert book.report("packed") == {"way": "packed", "packed_ms": 0.3891, "float_ms": None}
    for s in (1.0, 1.0, 0.00041237891):
        book.record("float", s)
    assert book.report("float") == {"way": "float", "packed_ms": 0.3891, "float_ms": 0.4124}
