"""The return code of every batch-source entry point for every kind of bad argument, pinned as a literal table.

The six dctn_batch_draw* / dctn_batch_gather* entry points are conveniences over dctn_batch_draw_call /
dctn_batch_gather_call (include/dctn_amd.h, version 513), and one planner holds the checks of all of them.  TABLE holds
what the library of version 512 - the last one in which each of the three source files checked its own arguments -
returned: for every single bad argument of the three `test_entry_points_validate_their_arguments_without_a_device` tests,
and for every pair drawn from one representative of each class (a NULL pointer, a bad shape, a bad dtype, an unsupported
width or region).  `python -m tests.test_host_batch_call_errors LIBRARY` prints the table of any library.  Every call here
returns before a launch: no GPU."""
import ctypes
import itertools
import sys

import pytest

from dctn_amd import _lib

P = 64   # a non-null dummy pointer: no call here gets as far as using one
NULL, SHAPE, DTYPE, UNSUPPORTED = _lib.ERR_NULL, _lib.ERR_BAD_SHAPE, _lib.ERR_BAD_DTYPE, _lib.ERR_UNSUPPORTED
U8, ROWS, COLOUR = _lib.BATCH_SRC_U8_TABLE, _lib.BATCH_SRC_ROWS, _lib.BATCH_SRC_COLOUR
IDENTITY, PAD, HFLIP = _lib.BATCH_IDENTITY_ORDER, _lib.BATCH_PAD_TAIL, _lib.AUG_HFLIP

_IN = ("src", "table", "labels")
_OUT = ("x", "y", "indices")
_DRAW = _IN + _OUT + ("state", "n", "global_batch", "count", "rank_offset")
_GATHER = _IN + ("sample_idx",) + _OUT + ("n", "count")
_AUG = ("flags", "dtype", "max_shift", "aug_flags", "fill", "stream")
# entry point -> its arguments in order, named as the fields of dctn_batch_call_t
ENTRY = {
    "dctn_batch_draw": _DRAW + ("row_len", "width", "src_kind", "flags", "dtype", "stream"),
    "dctn_batch_gather": _GATHER + ("row_len", "width", "src_kind", "dtype", "stream"),
    "dctn_batch_draw_cols": _DRAW + ("row_len", "src_channels", "width", "flags", "dtype", "stream"),
    "dctn_batch_gather_cols": _GATHER + ("row_len", "src_channels", "width", "dtype", "stream"),
    "dctn_batch_draw_aug": _DRAW + ("height", "width_px", "width") + _AUG,
    "dctn_batch_draw_cols_aug": _DRAW + ("height", "width_px", "src_channels", "width") + _AUG,
}
# a valid call but for the overrides of a case (the shapes of the three older tests)
VALID = dict(src=P, table=P, labels=P, sample_idx=P, x=P, y=P, indices=P, state=P, n=37, global_batch=8, count=8,
             rank_offset=0, row_len=25, height=5, width_px=7, src_kind=U8, flags=0, dtype=_lib.F32, max_shift=2,
             aug_flags=HFLIP, fill=0, stream=None)
WIDTHS = {name: dict(src_channels=3, width=4) if "cols" in name else dict(width=2) for name in ENTRY}

_SHARD = [dict(n=0), dict(n=1 << 31), dict(n=7), dict(global_batch=0, count=0), dict(count=0),
          dict(count=4, rank_offset=5), dict(count=4, rank_offset=-1)]
_COLS_WIDTHS = [dict(src_channels=5, width=5), dict(src_channels=3, width=2), dict(src_channels=4, width=5)]
_AUG_SINGLES = _SHARD + [
    dict(height=0), dict(width_px=0), dict(height=-3), dict(height=1 << 31), dict(width_px=1 << 31),
    dict(height=1 << 16, width_px=1 << 15), dict(width=0), dict(flags=PAD), dict(flags=IDENTITY | PAD), dict(flags=4),
    dict(flags=IDENTITY | 8), dict(max_shift=-1), dict(max_shift=1 << 15), dict(aug_flags=2), dict(aug_flags=HFLIP | 4),
    dict(dtype=7), dict(dtype=-1), dict(width=5), dict(src=None, n=0, dtype=7, width=5), dict(n=0, dtype=7, width=5),
    dict(max_shift=-1, dtype=7, width=5), dict(flags=PAD, dtype=7, width=5), dict(aug_flags=2, dtype=7, width=5),
    dict(dtype=7, width=5), dict(dtype=7, height=128, width_px=128), dict(height=128, width_px=128)]
# what the three older tests break, one call each
SINGLES = {
    "dctn_batch_draw": _SHARD + [dict(row_len=0), dict(src_kind=2), dict(flags=2), dict(width=5),
                                 dict(width=5, src_kind=ROWS, table=None), dict(dtype=7)],
    "dctn_batch_gather": [dict(n=0), dict(n=1 << 31), dict(count=0), dict(width=0), dict(src_kind=-1), dict(width=5),
                          dict(dtype=3)],
    "dctn_batch_draw_cols": _SHARD + [dict(row_len=0), dict(row_len=1 << 31), dict(src_channels=0, width=1),
                                      dict(src_channels=3, width=0), dict(src_channels=5, width=4),
                                      dict(src_channels=2, width=4)] + _COLS_WIDTHS + [
        dict(flags=4), dict(flags=IDENTITY | PAD | 4), dict(flags=PAD), dict(dtype=7), dict(dtype=-1),
        dict(n=0, dtype=7, width=5), dict(dtype=7, width=5)],
    "dctn_batch_gather_cols": [dict(n=0), dict(n=1 << 31), dict(count=0), dict(row_len=0), dict(src_channels=0, width=1),
                               dict(src_channels=-1, width=1), dict(src_channels=1, width=3)] + _COLS_WIDTHS + [dict(dtype=3)],
    "dctn_batch_draw_aug": _AUG_SINGLES + [dict(fill=0x100), dict(fill=0x80000000), dict(height=1, width_px=13 * 1024 + 1)],
    "dctn_batch_draw_cols_aug": _AUG_SINGLES + [
        dict(fill=0x01000000), dict(src_channels=1, width=2, fill=0xFF00), dict(fill=0x01000000, dtype=7),
        dict(src_channels=0, width=1), dict(src_channels=-1, width=1), dict(src_channels=2, width=4)] + _COLS_WIDTHS + [
        dict(height=67, width_px=67), dict(height=64, width_px=64, dtype=7), dict(height=64, width_px=64, width=5),
        dict(height=64, width_px=64, src_channels=5, width=5)],
}
# one representative of each class, for the pairs; and what decides between the kind and the table in the two plain forms
CLASSES = [dict(labels=None), dict(n=0), dict(dtype=7), dict(width=5)]
REGION = dict(height=128, width_px=128)
KIND_AND_TABLE = [dict(table=None, src_kind=2), dict(src=None, src_kind=2), dict(table=None, n=0),
                  dict(table=None, src_kind=ROWS, n=0), dict(table=None, src_kind=-1, dtype=7)]


def label(broken):
    return " & ".join(f"{k}={v}" for k, v in broken.items())


def cases(name):
    """case -> the arguments it breaks: every pointer, the singles of the older tests, then the pairs."""
    out = {f"{p}=None": {p: None} for p in ENTRY[name] if VALID.get(p) == P}
    out.update({label(b): b for b in SINGLES[name]})
    classes = CLASSES + ([REGION] if "aug" in name else [])
    for a, b in itertools.combinations(classes, 2):
        if not set(a) & set(b):
            out[label({**a, **b})] = {**a, **b}
    if name in ("dctn_batch_draw", "dctn_batch_gather"):
        out.update({label(b): b for b in KIND_AND_TABLE})
    return out


def values(name, broken):
    return {**VALID, **WIDTHS[name], **broken}


def legacy_call(lib, name, broken):
    v = values(name, broken)
    return getattr(lib, name)(*[v[a] for a in ENTRY[name]])


def descriptor_call(lib, name, broken):
    """The same call through dctn_batch_call_t: the kind and the augmentation the entry point's name implies."""
    v = values(name, broken)
    v["augment"] = int("aug" in name)
    if "cols" in name:
        v["src_kind"] = COLOUR
    if "aug" in name:
        v["row_len"] = v["height"] * v["width_px"]
    draw = "draw" in name
    v["sample_idx" if draw else "state"] = None   # the other operation's pointer is not looked at
    call = _lib.BatchCall(**{f: v.get(f, 0) for f, _ in _lib.BatchCall._fields_})
    return (lib.dctn_batch_draw_call if draw else lib.dctn_batch_gather_call)(ctypes.byref(call), None)


# what version 512 returned
TABLE = {
    "dctn_batch_draw": {
        "src=None": -6,
        "table=None": -6,
        "labels=None": -6,
        "x=None": -6,
        "y=None": -6,
        "indices=None": -6,
        "state=None": -6,
        "n=0": -1,
        "n=2147483648": -1,
        "n=7": -1,
        "global_batch=0 & count=0": -1,
        "count=0": -1,
        "count=4 & rank_offset=5": -1,
        "count=4 & rank_offset=-1": -1,
        "row_len=0": -1,
        "src_kind=2": -1,
        "flags=2": -1,
        "width=5": -3,
        "width=5 & src_kind=1 & table=None": -3,
        "dtype=7": -2,
        "labels=None & n=0": -6,
        "labels=None & dtype=7": -6,
        "labels=None & width=5": -6,
        "n=0 & dtype=7": -1,
        "n=0 & width=5": -1,
        "dtype=7 & width=5": -2,
        "table=None & src_kind=2": -1,
        "src=None & src_kind=2": -6,
        "table=None & n=0": -6,
        "table=None & src_kind=1 & n=0": -1,
        "table=None & src_kind=-1 & dtype=7": -1,
    },
    "dctn_batch_gather": {
        "src=None": -6,
        "table=None": -6,
        "labels=None": -6,
        "sample_idx=None": -6,
        "x=None": -6,
        "y=None": -6,
        "indices=None": -6,
        "n=0": -1,
        "n=2147483648": -1,
        "count=0": -1,
        "width=0": -1,
        "src_kind=-1": -1,
        "width=5": -3,
        "dtype=3": -2,
        "labels=None & n=0": -6,
        "labels=None & dtype=7": -6,
        "labels=None & width=5": -6,
        "n=0 & dtype=7": -1,
        "n=0 & width=5": -1,
        "dtype=7 & width=5": -2,
        "table=None & src_kind=2": -1,
        "src=None & src_kind=2": -6,
        "table=None & n=0": -6,
        "table=None & src_kind=1 & n=0": -1,
        "table=None & src_kind=-1 & dtype=7": -1,
    },
    "dctn_batch_draw_cols": {
        "src=None": -6,
        "table=None": -6,
        "labels=None": -6,
        "x=None": -6,
        "y=None": -6,
        "indices=None": -6,
        "state=None": -6,
        "n=0": -1,
        "n=2147483648": -1,
        "n=7": -1,
        "global_batch=0 & count=0": -1,
        "count=0": -1,
        "count=4 & rank_offset=5": -1,
        "count=4 & rank_offset=-1": -1,
        "row_len=0": -1,
        "row_len=2147483648": -1,
        "src_channels=0 & width=1": -1,
        "src_channels=3 & width=0": -1,
        "src_channels=5 & width=4": -3,
        "src_channels=2 & width=4": -3,
        "src_channels=5 & width=5": -3,
        "src_channels=3 & width=2": -3,
        "src_channels=4 & width=5": -3,
        "flags=4": -1,
        "flags=7": -1,
        "flags=2": -1,
        "dtype=7": -2,
        "dtype=-1": -2,
        "n=0 & dtype=7 & width=5": -1,
        "dtype=7 & width=5": -2,
        "labels=None & n=0": -6,
        "labels=None & dtype=7": -6,
        "labels=None & width=5": -6,
        "n=0 & dtype=7": -1,
        "n=0 & width=5": -1,
    },
    "dctn_batch_gather_cols": {
        "src=None": -6,
        "table=None": -6,
        "labels=None": -6,
        "sample_idx=None": -6,
        "x=None": -6,
        "y=None": -6,
        "indices=None": -6,
        "n=0": -1,
        "n=2147483648": -1,
        "count=0": -1,
        "row_len=0": -1,
        "src_channels=0 & width=1": -1,
        "src_channels=-1 & width=1": -1,
        "src_channels=1 & width=3": -3,
        "src_channels=5 & width=5": -3,
        "src_channels=3 & width=2": -3,
        "src_channels=4 & width=5": -3,
        "dtype=3": -2,
        "labels=None & n=0": -6,
        "labels=None & dtype=7": -6,
        "labels=None & width=5": -6,
        "n=0 & dtype=7": -1,
        "n=0 & width=5": -1,
        "dtype=7 & width=5": -2,
    },
    "dctn_batch_draw_aug": {
        "src=None": -6,
        "table=None": -6,
        "labels=None": -6,
        "x=None": -6,
        "y=None": -6,
        "indices=None": -6,
        "state=None": -6,
        "n=0": -1,
        "n=2147483648": -1,
        "n=7": -1,
        "global_batch=0 & count=0": -1,
        "count=0": -1,
        "count=4 & rank_offset=5": -1,
        "count=4 & rank_offset=-1": -1,
        "height=0": -1,
        "width_px=0": -1,
        "height=-3": -1,
        "height=2147483648": -1,
        "width_px=2147483648": -1,
        "height=65536 & width_px=32768": -1,
        "width=0": -1,
        "flags=2": -1,
        "flags=3": -1,
        "flags=4": -1,
        "flags=9": -1,
        "max_shift=-1": -1,
        "max_shift=32768": -1,
        "aug_flags=2": -1,
        "aug_flags=5": -1,
        "dtype=7": -2,
        "dtype=-1": -2,
        "width=5": -3,
        "src=None & n=0 & dtype=7 & width=5": -6,
        "n=0 & dtype=7 & width=5": -1,
        "max_shift=-1 & dtype=7 & width=5": -1,
        "flags=2 & dtype=7 & width=5": -1,
        "aug_flags=2 & dtype=7 & width=5": -1,
        "dtype=7 & width=5": -2,
        "dtype=7 & height=128 & width_px=128": -2,
        "height=128 & width_px=128": -3,
        "fill=256": -1,
        "fill=2147483648": -1,
        "height=1 & width_px=13313": -3,
        "labels=None & n=0": -6,
        "labels=None & dtype=7": -6,
        "labels=None & width=5": -6,
        "labels=None & height=128 & width_px=128": -6,
        "n=0 & dtype=7": -1,
        "n=0 & width=5": -1,
        "n=0 & height=128 & width_px=128": -1,
        "width=5 & height=128 & width_px=128": -3,
    },
    "dctn_batch_draw_cols_aug": {
        "src=None": -6,
        "table=None": -6,
        "labels=None": -6,
        "x=None": -6,
        "y=None": -6,
        "indices=None": -6,
        "state=None": -6,
        "n=0": -1,
        "n=2147483648": -1,
        "n=7": -1,
        "global_batch=0 & count=0": -1,
        "count=0": -1,
        "count=4 & rank_offset=5": -1,
        "count=4 & rank_offset=-1": -1,
        "height=0": -1,
        "width_px=0": -1,
        "height=-3": -1,
        "height=2147483648": -1,
        "width_px=2147483648": -1,
        "height=65536 & width_px=32768": -1,
        "width=0": -1,
        "flags=2": -1,
        "flags=3": -1,
        "flags=4": -1,
        "flags=9": -1,
        "max_shift=-1": -1,
        "max_shift=32768": -1,
        "aug_flags=2": -1,
        "aug_flags=5": -1,
        "dtype=7": -2,
        "dtype=-1": -2,
        "width=5": -3,
        "src=None & n=0 & dtype=7 & width=5": -6,
        "n=0 & dtype=7 & width=5": -1,
        "max_shift=-1 & dtype=7 & width=5": -1,
        "flags=2 & dtype=7 & width=5": -1,
        "aug_flags=2 & dtype=7 & width=5": -1,
        "dtype=7 & width=5": -2,
        "dtype=7 & height=128 & width_px=128": -2,
        "height=128 & width_px=128": -3,
        "fill=16777216": -1,
        "src_channels=1 & width=2 & fill=65280": -1,
        "fill=16777216 & dtype=7": -1,
        "src_channels=0 & width=1": -1,
        "src_channels=-1 & width=1": -1,
        "src_channels=2 & width=4": -3,
        "src_channels=5 & width=5": -3,
        "src_channels=3 & width=2": -3,
        "src_channels=4 & width=5": -3,
        "height=67 & width_px=67": -3,
        "height=64 & width_px=64 & dtype=7": -2,
        "height=64 & width_px=64 & width=5": -3,
        "height=64 & width_px=64 & src_channels=5 & width=5": -3,
        "labels=None & n=0": -6,
        "labels=None & dtype=7": -6,
        "labels=None & width=5": -6,
        "labels=None & height=128 & width_px=128": -6,
        "n=0 & dtype=7": -1,
        "n=0 & width=5": -1,
        "n=0 & height=128 & width_px=128": -1,
        "width=5 & height=128 & width_px=128": -3,
    },
}


def _bound(path):
    lib = ctypes.CDLL(path)
    for name in ENTRY:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_the_older_entry_points_answer_as_they_did(name):
    assert sorted(TABLE[name]) == sorted(cases(name))
    got = {case: legacy_call(_lib.lib(), name, broken) for case, broken in cases(name).items()}
    assert got == TABLE[name]
    assert all(code in (NULL, SHAPE, DTYPE, UNSUPPORTED) for code in got.values())   # nothing here reached a launch


def test_the_table_holds_every_class_every_pair_and_the_one_precedence_that_is_not_by_class():
    for name in ENTRY:
        t = TABLE[name]
        assert set(t.values()) == {NULL, SHAPE, DTYPE, UNSUPPORTED}
        # null, then shape, then dtype, then unsupported
        assert t["labels=None & n=0"] == t["labels=None & dtype=7"] == t["labels=None & width=5"] == NULL
        assert t["n=0 & dtype=7"] == t["n=0 & width=5"] == SHAPE and t["dtype=7 & width=5"] == DTYPE
        if "aug" in name:
            assert t["table=None"] == NULL   # an augmented draw always has a table
            assert t["n=0 & height=128 & width_px=128"] == SHAPE and t["dtype=7 & height=128 & width_px=128"] == DTYPE
            assert t["labels=None & height=128 & width_px=128"] == NULL and t["height=128 & width_px=128"] == UNSUPPORTED
    for name in ("dctn_batch_draw", "dctn_batch_gather"):
        t = TABLE[name]   # the kind says whether there is a table: it is answered behind the other pointers, in front of it
        assert t["table=None & src_kind=2"] == SHAPE and t["src=None & src_kind=2"] == NULL and t["table=None & n=0"] == NULL
        assert t["table=None & src_kind=1 & n=0"] == SHAPE and t["table=None & src_kind=-1 & dtype=7"] == SHAPE


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_the_descriptor_entry_points_answer_the_same(name):
    """The equivalent descriptor for every case of the table.  Left out: src_kind = 2 through dctn_batch_draw /
    dctn_batch_gather, which those two refuse as an unknown kind and the descriptor reads as the colour source."""
    lib = _lib.lib()
    ran = 0
    for case, broken in cases(name).items():
        if "cols" not in name and broken.get("src_kind") == COLOUR:
            continue
        assert descriptor_call(lib, name, broken) == TABLE[name][case], (name, case)
        ran += 1
    assert ran >= len(TABLE[name]) - 3


def test_what_only_the_descriptor_can_say():
    lib = _lib.lib()
    assert lib.dctn_batch_call_bytes() == ctypes.sizeof(_lib.BatchCall) == 160
    assert lib.dctn_batch_draw_call(None, None) == NULL and lib.dctn_batch_gather_call(None, None) == NULL

    def call(draw, **fields):   # a valid launch but for `fields`
        v = {**VALID, "width": 2, "src_channels": 0, "augment": 0, **fields}
        c = _lib.BatchCall(**{f: v[f] for f, _ in _lib.BatchCall._fields_})
        return (lib.dctn_batch_draw_call if draw else lib.dctn_batch_gather_call)(ctypes.byref(c), None)

    aug = dict(augment=1, row_len=35)
    assert call(False, **aug) == SHAPE                                        # there is no augmented gather
    assert call(False, **aug, src_kind=COLOUR, src_channels=3, width=4) == SHAPE
    assert call(False, **aug, table=None) == SHAPE and call(False, **aug, labels=None) == NULL
    assert call(True, **aug, src_kind=ROWS) == SHAPE                          # rows have no height and width
    assert call(True, augment=1, row_len=36) == SHAPE                             # row_len is height * width_px
    for draw in (True, False):
        for kind in (3, -1, 1 << 20):
            assert call(draw, src_kind=kind) == SHAPE
            assert call(draw, src_kind=kind, table=None) == SHAPE and call(draw, src_kind=kind, y=None) == NULL
            assert call(draw, src_kind=kind, dtype=7, width=5) == SHAPE
        # the colour source by its kind: its table and its two widths
        assert call(draw, src_kind=COLOUR, src_channels=3, width=4, table=None) == NULL
        assert call(draw, src_kind=COLOUR, src_channels=0, width=1) == SHAPE
        assert call(draw, src_kind=COLOUR, src_channels=3, width=2) == UNSUPPORTED
        assert call(draw, src_kind=COLOUR, src_channels=3, width=2, dtype=7) == DTYPE
    # what an operation or a kind ignores may hold anything
    assert call(True, n=0, sample_idx=None) == SHAPE and call(False, n=0, state=None) == SHAPE
    assert call(False, n=0, global_batch=0, rank_offset=-1, flags=64) == SHAPE
    assert call(False, dtype=7, global_batch=0, rank_offset=-1, flags=64, height=-1, max_shift=-1, fill=1 << 31) == DTYPE
    assert call(True, dtype=7, src_channels=9, height=-1, width_px=0, max_shift=-1, aug_flags=8, fill=1 << 31) == DTYPE


if __name__ == "__main__":
    library = _bound(sys.argv[1])
    for entry in ENTRY:
        print(f'    "{entry}": {{')
        for case_name, broken_args in cases(entry).items():
            print(f'        "{case_name}": {legacy_call(library, entry, broken_args)},')
        print("    },")
