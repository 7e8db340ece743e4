"""Constructed selection and NULL patterns for filter() on resident records (tests/test_gpu_filter_edges.py runs them on the device,
tests/test_filter_cases_cpu.py checks the builders themselves). Pure numpy / pyarrow, no GPU import.

The compaction works in tiles of 2 048 rows (one wave), steps of 512 (8-byte columns) or 1 024 rows (4-byte columns), groups of 64
rows, bitmap words of 32 rows, and a workgroup's share of four tiles: the row counts sit around each of these, and the selection
patterns put the selected rows where a path changes — nothing, everything, a tile's or a record's first and last row, empty steps and
empty tiles, and runs that move the output's bit offset.

One record layout for every case. Every value is a function of the record's number and the row's number, so a misplaced row names itself:
  sel    int64, never NULL       1 where the row is selected, else 0: the predicate `sel > 0` (8 bytes: the one-pass kernel by default)
  selk   dictionary, never NULL  "y" / "n": the predicate `selk == "y"` (4 bytes: one pass only when asked for)
  seln   int64 with NULLs        as sel, NULL in rows r mod 7 = 3: a filter column that cannot be fused (`seln > 0` selects less)
  d      dictionary, nullable    entry r mod 251 of 251
  k      dictionary, never NULL  entry r mod 241 of 241
  i      int64, nullable         record x 2^20 + r
  f      float64, never NULL     i + 0.5
  flag   bool, nullable          r mod 3 = 0
  plain  binary, nullable        b"p<r mod 97>"
The validity pattern of a case applies to d, i, flag and plain alike."""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import numpy as np
import pyarrow as pa

TILE, GROUP, WORD, SHARE_TILES = 2048, 64, 32, 4
STEPS = (512, 1024)

ROWS = [1, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097,
        6145,  # three tiles and one row: the share's fourth tile and most of the third tile's steps lie past the end
        8191, 8192, 8193]

SELECTIONS = ["none", "all", "first_row", "last_row", "tile_first_rows", "tile_last_rows", "group_edges", "all_but_one_per_tile",
              "alternate_tiles", "runs_65_63", "bernoulli_50", "bernoulli_1"]
BERNOULLI = {"bernoulli_50": 0.5, "bernoulli_1": 0.01}

VALIDITIES = ["no_bitmap", "one_null_unselected", "null_where_selected", "null_where_unselected", "group_last_rows", "bernoulli_3", "all_null"]
NULLABLE_COLUMNS = ["d", "i", "flag", "plain"]
COLUMNS = ["sel", "selk", "seln", "d", "k", "i", "f", "flag", "plain"]

LEADS = range(64)
LEAD_ROWS = 2049


def selection(name: str, n: int, lead: int = 0) -> np.ndarray:
    """The boolean mask of pattern `name` over an n-row record. `lead` (runs_65_63 only): that many selected rows in front of the runs."""
    r = np.arange(n, dtype=np.int64)
    if name == "none":
        return np.zeros(n, dtype=bool)
    if name == "all":
        return np.ones(n, dtype=bool)
    if name == "first_row":
        return r == 0
    if name == "last_row":
        return r == n - 1
    if name == "tile_first_rows":
        return r % TILE == 0
    if name == "tile_last_rows":  # (the record's last row is the last row of its last tile)
        return (r % TILE == TILE - 1) | (r == n - 1)
    if name == "group_edges":
        return (r % GROUP == 0) | (r % GROUP == GROUP - 1)
    if name == "all_but_one_per_tile":
        return r % TILE != 1000
    if name == "alternate_tiles":
        return (r // TILE) % 2 == 0
    if name == "runs_65_63":  # runs of 65 selected rows, then 63 that are not
        return (r < lead) | ((r >= lead) & ((r - lead) % 128 < 65))
    if name in BERNOULLI:
        return np.random.default_rng(1000 * n + SELECTIONS.index(name)).random(n) < BERNOULLI[name]
    raise KeyError(name)


def selected_count(name: str, n: int, lead: int = 0) -> Optional[int]:
    """The number of selected rows in closed form; None for the random patterns."""
    q, rem = divmod(n, TILE)
    if name == "none":
        return 0
    if name == "all":
        return n
    if name in ("first_row", "last_row"):
        return 1
    if name in ("tile_first_rows", "tile_last_rows"):
        return (n + TILE - 1) // TILE
    if name == "group_edges":
        return (n + GROUP - 1) // GROUP + n // GROUP
    if name == "all_but_one_per_tile":
        return n - (n + TILE - 1001) // TILE
    if name == "alternate_tiles":
        return (q + 1) // 2 * TILE + (rem if q % 2 == 0 else 0)
    if name == "runs_65_63":
        m = max(n - lead, 0)
        return min(lead, n) + m // 128 * 65 + min(m % 128, 65)
    return None


def validity(name: str, n: int, mask: np.ndarray) -> Optional[np.ndarray]:
    """Which rows of the nullable columns are valid (None: the columns carry no bitmap)."""
    r = np.arange(n, dtype=np.int64)
    if name == "no_bitmap":
        return None
    if name == "one_null_unselected":  # a bitmap is there and every step is all-valid; a record without an unselected row has no NULL
        off = np.flatnonzero(~mask)
        if len(off) == 0:
            return None
        v = np.ones(n, dtype=bool)
        v[off[len(off) // 2]] = False
        return v
    if name == "null_where_selected":
        return ~mask
    if name == "null_where_unselected":
        return mask.copy()
    if name == "group_last_rows":
        return r % GROUP != GROUP - 1
    if name == "bernoulli_3":
        return np.random.default_rng(77 * n + 5).random(n) >= 0.03
    if name == "all_null":
        return np.zeros(n, dtype=bool)
    raise KeyError(name)


SELN_NULL = lambda n: np.arange(n) % 7 == 3  # noqa: E731

DICT_TYPE = pa.dictionary(pa.uint32(), pa.binary())
_D = pa.array([b"d%03d" % j for j in range(251)], type=pa.binary())
_K = pa.array([b"k%03d" % j for j in range(241)], type=pa.binary())
_P = pa.array([b"p%d" % j for j in range(97)], type=pa.binary())
_YN = pa.array([b"n", b"y"], type=pa.binary())


def record(rec: int, mask: np.ndarray, valid: Optional[np.ndarray]) -> pa.RecordBatch:
    """Record number `rec` of the layout above for the selection `mask` and the validity `valid`."""
    n = len(mask)
    r = np.arange(n, dtype=np.int64)
    null = None if valid is None else ~valid
    i = rec * (1 << 20) + r
    sel = mask.astype(np.int64)
    arrays = [
        pa.array(sel),
        pa.DictionaryArray.from_arrays(pa.array(mask.astype(np.uint32)), _YN),
        pa.array(sel, mask=SELN_NULL(n)),
        pa.DictionaryArray.from_arrays(pa.array((r % 251).astype(np.uint32), mask=null), _D),
        pa.DictionaryArray.from_arrays(pa.array((r % 241).astype(np.uint32)), _K),
        pa.array(i, mask=null),
        pa.array(i + 0.5),
        pa.array(r % 3 == 0, mask=null),
        pa.DictionaryArray.from_arrays(pa.array((r % 97).astype(np.uint32), mask=null), _P).cast(pa.binary()),
    ]
    return pa.RecordBatch.from_arrays(arrays, names=COLUMNS)


class Case(NamedTuple):
    rows: int
    selection: str
    lead: int
    mask: np.ndarray


def grid() -> List[Case]:
    """The records of one packed launch: every row count with every selection pattern, then the 65 / 63 runs behind 0 … 63 selected
    rows (LEAD_ROWS rows each). A step of 512 rows holds four whole runs, 260 rows, whatever comes before it: without the leads
    the output's bit offset at a step's start — what the validity bits are shifted by — would only ever be a multiple of 4."""
    cases = [Case(n, s, 0, selection(s, n)) for n in ROWS for s in SELECTIONS]
    cases += [Case(LEAD_ROWS, "runs_65_63", lead, selection("runs_65_63", LEAD_ROWS, lead)) for lead in LEADS if lead > 0]
    return cases


def step_start_offsets(mask: np.ndarray, step: int) -> set:
    """Output bit offsets (mod 64) at the start of every step that selects a row."""
    before = np.concatenate([[0], np.cumsum(mask)])
    return {int(before[s]) % 64 for s in range(0, len(mask), step) if before[min(s + step, len(mask))] > before[s]}


def threshold_counts(n: int) -> List[int]:
    """Selected-row counts around the 40 % repack threshold of the fused columns (a result is repacked when selected < 0.4 n)."""
    c = -(-2 * n // 5)  # ⌈0.4 n⌉
    return [0, c - 1, c, c + 1, n]


def spread_mask(n: int, count: int) -> np.ndarray:
    """`count` selected rows spread evenly over n."""
    m = np.zeros(n, dtype=bool)
    if count > 0:
        m[(np.arange(count, dtype=np.int64) * n) // count] = True
    return m


def mask_of(rec: pa.RecordBatch, column: str) -> np.ndarray:
    """The rows the predicate on `column` (sel > 0, selk == "y", seln > 0) selects."""
    if column == "selk":
        return rec.column("selk").indices.to_numpy() == 1
    c = rec.column(column)
    return np.asarray(c.fill_null(0)) > 0
