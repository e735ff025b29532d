"""Change points with credible intervals from the joint trajectories.

The backward kernel's output is P = B x seeds joint draws of the whole state
path, durations included. A change point whose location is uncertain by a few
sites is significant at no single site; "is there a change point in this
window?" is a statement about the joint path and is answered, over that
sample, by counting trajectories. The reference pipeline has no caller of
change points.

For a site t that is not its group's first row, against row t - 1 of the same
trajectory, a (d, r) state *continues* when r is unchanged and d is one more
modulo 2^16. Event kinds (the columns of the event matrix): 0 control and
1 case (the group's state does not continue), 2 any (0 or 1), 3 split
(merged != 0 -> == 0), 4 merge (merged == 0 -> != 0).

Device-side functions (C ABI hyg_cp_*, include/hygeia_amd.h), usable straight
on a launch's outputs in HBM, device tensors in and out like dmr.py:

  site_events()       c_t of the five kinds -> [n_sites][5] int32
  find_windows()      maximal runs of linked sites with c_t >= min_count of one
                      kind (dmr.find_regions on the event matrix)
  window_counts()     per window: trajectories with at least one event (n_any)
                      and with exactly one (n_one)
  window_intervals()  per window: events, modal site, and the central interval
                      [lo, hi] of the events' locations at a rational level

and the command `hygeia get_change_points` on `hygeia aggregate`'s matrices.
There is no CPU path: without the HIP library or a GPU these functions raise.
"""
from __future__ import annotations

import ctypes as C
import os
from fractions import Fraction
from pathlib import Path
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from .dmp import _torch, fdr, site_counts
from .dmr import MAX_FRACTION_DENOMINATOR, _fraction, _sp, find_regions, min_count_of, region_sums

KINDS = ("control", "case", "any", "split", "merge")
N_KINDS = len(KINDS)


def _groups_args(groups, block_rows):
    n_groups = len(groups)
    n_seeds = len(block_rows[0]) if n_groups else 1
    g_arr = (_lib.DmpGroup * max(n_groups, 1))(*[_lib.DmpGroup(int(a), int(b)) for a, b in groups])
    br = np.ascontiguousarray(np.asarray(block_rows, dtype=np.int64).reshape(-1))
    return g_arr, br, br.ctypes.data_as(C.POINTER(C.c_int64)), n_groups, n_seeds


def _check_trajectories(torch, arrays):
    dev = next(a for a in arrays if a is not None).device
    for a in arrays:
        if a is not None and (a.dtype != torch.int16 or not a.is_contiguous() or a.device != dev):
            raise ValueError("merged/control/kase must be contiguous int16 tensors on one device")
    return dev


def site_events(merged, control, kase, B: int, groups: Sequence[Tuple[int, int]],
                block_rows: Sequence[Sequence[int]], n_sites: int, events=None, stream=None):
    """c_t of the five event kinds: a device [n_sites][5] int32 tensor.

    merged [rows][B] (or None: columns 3 and 4 are 0), control / kase
    [rows][B][2] int16 (hyg_tg_outputs layout), groups and block_rows as
    dmp.site_counts (sorted by site, disjoint). A group's first row has no
    event; rows of sites outside the groups are not written (0 in a tensor
    made here)."""
    torch = _torch()
    dev = _check_trajectories(torch, (merged, control, kase))
    if events is None:
        events = torch.zeros((n_sites, N_KINDS), dtype=torch.int32, device=dev)
    g_arr, br, br_p, n_groups, n_seeds = _groups_args(groups, block_rows)
    _lib.check(_lib.load().hyg_cp_site_events(
        merged.data_ptr() if merged is not None else None, control.data_ptr(), kase.data_ptr(), int(B), g_arr, br_p,
        n_groups, n_seeds, int(n_sites), events.data_ptr(), _sp(stream, dev)))
    return events


def find_windows(events, kind: int, min_count: int, positions, max_gap: int, stream=None):
    """Candidate windows of one kind: maximal runs of sites with c_t >=
    min_count whose neighbours lie 0 < gap <= max_gap apart, [n][2] int64
    (begin, end). With min_count >= 1 no window holds a group's first row."""
    return find_regions(events, int(kind), int(min_count), positions, int(max_gap), 1, stream=stream)


def window_counts(merged, control, kase, B: int, groups: Sequence[Tuple[int, int]],
                  block_rows: Sequence[Sequence[int]], n_sites: int, kind: int, windows, stream=None):
    """(n_any, n_one) of every window for one kind: a device [n][2] int32
    tensor. Kinds 0 to 2 read control / kase, kinds 3 and 4 read merged (which
    may be None for the others). Windows may span groups or uncovered sites."""
    torch = _torch()
    dev = _check_trajectories(torch, (merged, control, kase))
    if windows.dtype != torch.int64 or not windows.is_contiguous() or windows.device != dev:
        raise ValueError("windows must be a contiguous int64 tensor on the trajectories' device")
    n = int(windows.shape[0])
    out = torch.empty((n, 2), dtype=torch.int32, device=dev)
    g_arr, br, br_p, n_groups, n_seeds = _groups_args(groups, block_rows)
    _lib.check(_lib.load().hyg_cp_window_counts(
        merged.data_ptr() if merged is not None else None, control.data_ptr() if control is not None else None,
        kase.data_ptr() if kase is not None else None, int(B), g_arr, br_p, n_groups, n_seeds, int(n_sites),
        int(kind), windows.data_ptr() if n else None, n, out.data_ptr() if n else None, _sp(stream, dev)))
    return out


def window_intervals(events, column: int, windows, level, stream=None):
    """(n_events, mode, lo, hi) of every window from column `column` of the
    int32 device matrix events [n_sites][stride]: a device [n][4] int64
    tensor of absolute site indices. level: a fractions.Fraction, a (num, den)
    tuple or anything Fraction() takes, 0 < level <= 1, denominator <= 1000."""
    torch = _torch()
    dev = events.device
    if events.dtype != torch.int32 or events.dim() != 2 or not events.is_contiguous():
        raise ValueError("events must be a contiguous 2-D int32 tensor")
    if windows.dtype != torch.int64 or not windows.is_contiguous() or windows.device != dev:
        raise ValueError("windows must be a contiguous int64 tensor on events' device")
    num, den = _fraction(level)
    n = int(windows.shape[0])
    out = torch.empty((n, 4), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().hyg_cp_window_intervals(
        events.data_ptr(), int(events.shape[1]), int(column), int(events.shape[0]), windows.data_ptr() if n else None,
        n, num, den, out.data_ptr() if n else None, _sp(stream, dev)))
    return out


# ------------------------------------------------------- get_change_points
GET_CHANGE_POINTS_FLAGS = [
    ("results_dir", "string", os.path.join(Path(os.getcwd()).parents[0], "test"),
     "Directory of `hygeia aggregate`'s outputs (regimes, durations and merge states per chromosome)."),
    ("output_dir", "string", os.path.join(Path(os.getcwd()).parents[0], "test", "cp"),
     "Directory for the outputs of this script."),
    ("chroms", "string", "21", "The chromosomes to analyze, a comma list"),
    ("n_regimes", "int", 6, "number of regimes."),
    ("segment_size", "int", 100000, "rows of a batch (as infer): each batch is its own set of draws; 0 = one group"),
    ("fdr_thresholds", "multi_float", [.01, .05], "fdr threshold for selecting change points."),
    ("site_prob", "float", 0.05, "a window's sites have at least this fraction of trajectories with an event"),
    ("max_gap_bp", "int", 300, "largest distance between neighbouring sites of a window"),
    ("level", "string", "0.9", "level of the location interval (a decimal or a ratio such as 9/10)"),
]

OUTPUT_KINDS = (("control", 0), ("case", 1), ("split", 3), ("merge", 4))  # (file name, event kind)
COLUMNS = ("chrom", "start", "end", "n_sites", "n_any", "n_one", "n_events", "prob_any", "null_stat", "mode_pos",
           "lo_pos", "hi_pos", "regime_before", "regime_after")
SEGMENT_COLUMNS = ("chrom", "start", "end", "n_sites", "regime", "regime_share")


def parse_level(text: str) -> Fraction:
    """--level from the flag's text, exactly (fractions.Fraction), in (0, 1]."""
    from .cli import FlagError

    try:
        fr = Fraction(str(text).strip())
    except (ValueError, ZeroDivisionError) as e:
        raise FlagError(f"invalid value for --level: {text!r} ({e})")
    if fr <= 0 or fr > 1:
        raise FlagError(f"--level must lie in (0, 1]: {text!r}")
    if fr.denominator > MAX_FRACTION_DENOMINATOR:
        raise FlagError(f"--level {text!r} has the denominator {fr.denominator}, above {MAX_FRACTION_DENOMINATOR}")
    return fr


def groups_of(T: int, segment_size: int) -> List[Tuple[int, int]]:
    """aggregate concatenates the batches' rows: consecutive segment_size-row groups, the last one shorter."""
    if segment_size <= 0 or T == 0:
        return [(0, T)]
    return [(g0, min(segment_size, T - g0)) for g0 in range(0, T, segment_size)]


def _matrix(results_dir: str, name: str, chrom: str):
    import pandas as pd

    d = pd.read_csv(os.path.join(results_dir, f"{name}_chrom_{chrom}.csv.gz"), sep="\t").set_index("pos")
    return d.index.to_numpy().astype(np.int64), d.to_numpy()


def _states(regimes: np.ndarray, durations: np.ndarray, device):
    """[T][P] regimes and durations -> a (d, r) int16 trajectory block [T][P][2]."""
    st = np.empty(regimes.shape + (2,), dtype=np.int16)
    st[:, :, 0] = durations
    st[:, :, 1] = regimes
    return _torch().from_numpy(st).to(device)


def chromosome_windows(chrom: str, results_dir: str, K: int, segment_size: int, site_prob: float, max_gap: int,
                       level: Fraction, device):
    """One chromosome, resident once: (P, pos [T], groups, counts [T][2 + 2K]
    (hyg_dmp_site_counts' matrix, numpy), {kind name: (windows [n][2],
    (n_any, n_one) [n][2], (n_events, mode, lo, hi) [n][4])}, numpy)."""
    torch = _torch()
    pos, creg = _matrix(results_dir, "control_regimes", chrom)
    mats = [creg] + [_matrix(results_dir, n, chrom)[1] for n in
                     ("case_regimes", "control_durations", "case_durations", "merge_states")]
    if any(m.shape != creg.shape for m in mats):
        raise ValueError(f"chromosome {chrom}: the regime, duration and merge-state matrices differ in shape")
    T, P = creg.shape
    mc = min_count_of(site_prob, P)  # >= 1: the command refuses --site_prob 0
    c_dev, k_dev = _states(mats[0], mats[2], device), _states(mats[1], mats[3], device)
    m_dev = torch.from_numpy(np.ascontiguousarray(mats[4], dtype=np.int16)).to(device)
    groups = groups_of(T, segment_size)
    block_rows = [[g0] for g0, _ in groups]  # one seed block with B = P: a group's rows are the chromosome's
    counts, _ = site_counts(m_dev, c_dev, k_dev, P, K, groups, block_rows, T)
    events = site_events(m_dev, c_dev, k_dev, P, groups, block_rows, T)
    p_dev = torch.from_numpy(np.ascontiguousarray(pos)).to(device)
    out = {}
    for name, kind in OUTPUT_KINDS:
        w = find_windows(events, kind, mc, p_dev, max_gap).contiguous()
        wc = window_counts(m_dev, c_dev, k_dev, P, groups, block_rows, T, kind, w)
        wi = window_intervals(events, kind, w, level)
        out[name] = (w.cpu().numpy(), wc.cpu().numpy(), wi.cpu().numpy())
    torch.cuda.synchronize(device)
    return P, pos, groups, counts.cpu().numpy(), out


def _mode(hist) -> int:
    return int(np.argmax(hist)) + 1  # 1-based as Control_METEOR_{i+1}, ties to the lowest


def _rows(chrom, name, pos, counts, K: int, P: int, w, wc, wi) -> List[tuple]:
    off = 2 if name in ("control", "split") else 2 + K  # the control group's histogram, or the case group's
    rows = []
    for i in range(len(w)):
        a, b = int(w[i, 0]), int(w[i, 1])
        n_any = int(wc[i, 0])
        rows.append((chrom, int(pos[a]), int(pos[b - 1]), b - a, n_any, int(wc[i, 1]), int(wi[i, 0]), n_any / P,
                     1. - n_any / P, int(pos[wi[i, 1]]), int(pos[wi[i, 2]]), int(pos[wi[i, 3]]),
                     _mode(counts[a - 1, off:off + K]), _mode(counts[b - 1, off:off + K])))
    return rows


def segments_between(groups, windows) -> np.ndarray:
    """The stretches of each group between consecutive windows (ascending,
    each inside one group), empty ones dropped: [n][2] int64."""
    out, i, n = [], 0, len(windows)
    for g0, nr in groups:
        u, g1 = int(g0), int(g0) + int(nr)
        while i < n and int(windows[i][1]) <= g1:
            a, b = int(windows[i][0]), int(windows[i][1])
            if a > u:
                out.append((u, a))
            u = b
            i += 1
        if g1 > u:
            out.append((u, g1))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def _segment_rows(chrom, name, pos, counts, K: int, P: int, groups, windows, device) -> List[tuple]:
    torch = _torch()
    seg = segments_between(groups, windows)
    if not len(seg):
        return []
    sums = region_sums(torch.from_numpy(np.ascontiguousarray(counts)).to(device),
                       torch.from_numpy(seg).to(device)).cpu().numpy()
    off = 2 if name == "control" else 2 + K
    rows = []
    for i, (u, v) in enumerate(seg):
        h = sums[i, off:off + K]
        r = int(np.argmax(h))
        rows.append((chrom, int(pos[u]), int(pos[v - 1]), int(v - u), r + 1, int(h[r]) / (int(v - u) * P)))
    return rows


def _write(path: str, columns: Sequence[str], rows: Sequence[tuple]) -> None:
    with open(path, "w") as fh:
        fh.write("\t".join(columns) + "\n")
        for r in rows:
            fh.write("\t".join(repr(v) if isinstance(v, float) else str(v) for v in r) + "\n")


def get_change_points_main(argv: Sequence[str]) -> int:
    """`hygeia get_change_points`: per kind (control, case, split, merge) the
    candidate windows of every chromosome (one chromosome's matrices resident
    at a time), pooled; FDR_procedure on the pooled 1 - n_any / P per
    threshold; cp_{kind}_candidates.tsv, cp_{kind}_{thr}.tsv, and the
    segmentation between the selected windows, segments_{control,case}_{thr}.tsv.
    Each chromosome's per-site count matrix ([T][2 + 2K] int32) stays on the
    host until the selection is known."""
    import sys

    torch = _torch()
    from .cli import FlagError, parse_flags

    f = parse_flags(argv, GET_CHANGE_POINTS_FLAGS)
    K = int(f["n_regimes"])
    level = parse_level(f["level"])
    site_prob = float(f["site_prob"])
    if not 0. <= site_prob <= 1.:
        raise FlagError("--site_prob must lie in [0, 1]")
    if min_count_of(site_prob, 1) < 1:  # 0 / P >= site_prob, whatever P
        raise FlagError("--site_prob 0 admits sites without any event: a window needs min_count >= 1")
    if K < 1 or K > 16 or int(f["max_gap_bp"]) < 0 or int(f["segment_size"]) < 0:
        raise FlagError("--n_regimes must lie in [1, 16], --max_gap_bp and --segment_size must be >= 0")
    chroms = [c for c in str(f["chroms"]).split(",") if c != ""]
    if not chroms:
        raise FlagError("--chroms is empty")
    out_dir = f["output_dir"]
    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device("cuda", 0)
    P, per_chrom = None, []
    rows = {name: [] for name, _ in OUTPUT_KINDS}
    for chrom in chroms:
        Pc, pos, groups, counts, res = chromosome_windows(chrom, f["results_dir"], K, int(f["segment_size"]),
                                                          site_prob, int(f["max_gap_bp"]), level, dev)
        if P is not None and Pc != P:
            print(f"hygeia get_change_points: chromosome {chrom} has {Pc} trajectories, the chromosomes before it "
                  f"{P}", file=sys.stderr)
            return 1
        P = Pc
        for name, _ in OUTPUT_KINDS:
            w, wc, wi = res[name]
            rows[name].extend(_rows(chrom, name, pos, counts, K, P, w, wc, wi))
        per_chrom.append((chrom, pos, groups, counts, {n: res[n][0] for n in ("control", "case")}))
    for name, _ in OUTPUT_KINDS:
        rs = rows[name]
        _write(os.path.join(out_dir, f"cp_{name}_candidates.tsv"), COLUMNS, rs)
        if rs:
            n_any = np.array([r[4] for r in rs], dtype=np.int32)
            null_stat = 1. - n_any.astype(np.int64) / P
            pooled = torch.from_numpy(n_any.reshape(-1, 1).copy()).to(dev)
        for thr in f["fdr_thresholds"]:
            keep = np.zeros(len(rs), dtype=bool)
            if rs:
                _, _, threshold = fdr(pooled, 0, P, thr)
                keep = null_stat < threshold
            _write(os.path.join(out_dir, "cp_{}_{}.tsv".format(name, thr)), COLUMNS,
                   [r for r, k in zip(rs, keep) if k])
            if name not in ("control", "case"):
                continue
            seg_rows, o = [], 0
            for chrom, pos, groups, counts, wins in per_chrom:  # the rows are in the chromosomes' order
                w = wins[name]
                seg_rows.extend(_segment_rows(chrom, name, pos, counts, K, P, groups, w[keep[o:o + len(w)]], dev))
                o += len(w)
            _write(os.path.join(out_dir, "segments_{}_{}.tsv".format(name, thr)), SEGMENT_COLUMNS, seg_rows)
    return 0
