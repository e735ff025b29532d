"""Differentially methylated regions (DMRs) from the joint trajectories.

`hygeia get_dmps` tests single sites on the per-site statistic
1 - #(r_ctrl != r_case) / P. The backward kernel's output is more than that:
P = B x seeds joint draws of the whole state path. Whether a whole stretch is
differential is answered exactly, over that sample, by counting the
trajectories that are differential at every site (or at a given fraction of
the sites) of the stretch. The reference pipeline has no region caller.

Device-side functions (C ABI hyg_dmr_*, include/hygeia_amd.h), usable straight
on a launch's outputs in HBM, device tensors in and out like dmp.site_counts:

  find_regions()   candidate regions: maximal runs of seed sites (count >=
                   min_count) whose neighbours lie 0 < gap <= max_gap apart,
                   of at least min_sites sites -> [n][2] int64 (begin, end)
  region_counts()  per region, over its n sites, s_p = #differential sites of
                   trajectory p: n_all = #(s_p == n), n_frac = #(s_p >= f n)
  region_sums()    column sums of the per-site count matrix over each region

and the command `hygeia get_dmrs` on `hygeia aggregate`'s matrices. There is
no CPU path: without the HIP library or a GPU these functions raise.
"""
from __future__ import annotations

import ctypes as C
import os
from fractions import Fraction
from pathlib import Path
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from .dmp import _stream, _torch, _upload_regimes, fdr, site_counts

MAX_FRACTION_DENOMINATOR = 1000
_BOUND_BYTES = 64 << 20  # find_regions allocates its bound up to this size, else counts first


def _sp(stream, device):
    s = stream if stream is not None else _stream(device)
    return s if isinstance(s, C.c_void_p) else C.c_void_p(s)


def _fraction(fraction) -> Tuple[int, int]:
    fr = fraction if isinstance(fraction, Fraction) else (
        Fraction(*fraction) if isinstance(fraction, tuple) else Fraction(fraction))
    return fr.numerator, fr.denominator


def find_regions(counts, column: int, min_count: int, positions, max_gap: int, min_sites: int, stream=None):
    """Candidate regions of column `column` of the int32 device matrix counts
    [n_sites][stride] and the int64 device positions [n_sites]: a device
    [n][2] int64 tensor of (begin, end) site indices, ascending."""
    torch = _torch()
    dev = counts.device
    if counts.dtype != torch.int32 or counts.dim() != 2 or not counts.is_contiguous():
        raise ValueError("counts must be a contiguous 2-D int32 tensor")
    if positions.dtype != torch.int64 or not positions.is_contiguous() or positions.device != dev \
            or positions.numel() != counts.shape[0]:
        raise ValueError("positions must be a contiguous int64 tensor of counts' rows on counts' device")
    n_sites, stride = int(counts.shape[0]), int(counts.shape[1])
    L = _lib.load()
    s = _sp(stream, dev)
    n = C.c_int64()

    def call(buf, cap):
        return L.hyg_dmr_find_regions(counts.data_ptr(), stride, int(column), n_sites, int(min_count),
                                      positions.data_ptr(), int(max_gap), int(min_sites), buf, cap, C.byref(n), s)

    bound = n_sites // max(int(min_sites), 1)
    if bound * 16 > _BOUND_BYTES:  # count first, then allocate what is needed
        _lib.check(call(None, 0))
        bound = n.value
    regions = torch.empty((bound, 2), dtype=torch.int64, device=dev)
    _lib.check(call(regions.data_ptr() if bound else None, bound))
    return regions[:n.value]


def region_counts(control, kase, B: int, groups: Sequence[Tuple[int, int]], block_rows: Sequence[Sequence[int]],
                  n_sites: int, regions, fraction, stream=None):
    """(n_all, n_frac) of every region: a device [n_regions][2] int32 tensor.

    control / kase [rows][B][2] int16 (hyg_tg_outputs layout), groups and
    block_rows as dmp.site_counts (sorted by site, disjoint); regions a device
    [n][2] int64 tensor; fraction a fractions.Fraction, a (num, den) tuple or
    anything Fraction() takes, with a denominator of at most 1000."""
    torch = _torch()
    dev = control.device
    for a in (control, kase):
        if a.dtype != torch.int16 or not a.is_contiguous() or a.device != dev:
            raise ValueError("control/kase must be contiguous int16 tensors on one device")
    if regions.dtype != torch.int64 or not regions.is_contiguous() or regions.device != dev:
        raise ValueError("regions must be a contiguous int64 tensor on the trajectories' device")
    num, den = _fraction(fraction)
    n_regions = int(regions.shape[0])
    out = torch.empty((n_regions, 2), dtype=torch.int32, device=dev)
    n_groups = len(groups)
    n_seeds = len(block_rows[0]) if n_groups else 1
    g_arr = (_lib.DmpGroup * max(n_groups, 1))(*[_lib.DmpGroup(int(a), int(b)) for a, b in groups])
    br = np.ascontiguousarray(np.asarray(block_rows, dtype=np.int64).reshape(-1))
    _lib.check(_lib.load().hyg_dmr_region_counts(
        control.data_ptr(), kase.data_ptr(), int(B), g_arr, br.ctypes.data_as(C.POINTER(C.c_int64)), n_groups,
        n_seeds, int(n_sites), regions.data_ptr() if n_regions else None, n_regions, num, den,
        out.data_ptr() if n_regions else None, _sp(stream, dev)))
    return out


def region_sums(counts, regions, stream=None):
    """Column sums of the int32 device matrix counts [n_sites][stride] over
    each region: a device [n_regions][stride] int64 tensor."""
    torch = _torch()
    dev = counts.device
    if counts.dtype != torch.int32 or counts.dim() != 2 or not counts.is_contiguous():
        raise ValueError("counts must be a contiguous 2-D int32 tensor")
    if regions.dtype != torch.int64 or not regions.is_contiguous() or regions.device != dev:
        raise ValueError("regions must be a contiguous int64 tensor on counts' device")
    n_regions, stride = int(regions.shape[0]), int(counts.shape[1])
    out = torch.empty((n_regions, stride), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().hyg_dmr_region_sums(counts.data_ptr(), stride, int(counts.shape[0]),
                                               regions.data_ptr() if n_regions else None, n_regions,
                                               out.data_ptr() if n_regions else None, _sp(stream, dev)))
    return out


# ---------------------------------------------------------------- get_dmrs
GET_DMRS_FLAGS = [
    ("results_dir", "string", os.path.join(Path(os.getcwd()).parents[0], "test"),
     "Directory of `hygeia aggregate`'s outputs (control/case_regimes_chrom_{c}.csv.gz)."),
    ("output_dir", "string", os.path.join(Path(os.getcwd()).parents[0], "test", "dmr"),
     "Directory for the outputs of this script."),
    ("chroms", "string", "21", "The chromosomes to analyze, a comma list"),
    ("n_regimes", "int", 6, "number of regimes."),
    ("mu", "list", "0.95,0.05,0.80,0.20,0.50,0.50", "mu of the beta distribution (as infer)"),
    ("fdr_thresholds", "multi_float", [.01, .05], "fdr threshold for selecting DMRs."),
    ("site_prob", "float", 0.5, "a seed site has at least this fraction of differential trajectories"),
    ("max_gap_bp", "int", 300, "largest distance between neighbouring sites of a region"),
    ("min_sites", "int", 3, "fewest sites of a region"),
    ("min_fraction", "string", "0.8", "a trajectory supports a region when it is differential at this fraction of "
                                      "its sites (a decimal or a ratio such as 4/5)"),
]

COLUMNS = ("chrom", "start", "end", "n_sites", "n_all", "n_frac", "prob_all", "prob_frac", "null_stat",
           "mean_site_prob", "delta_mu", "control_regime", "case_regime")


def min_count_of(site_prob: float, P: int) -> int:
    """The smallest integer c in [0, P + 1] with c / P >= site_prob in float64."""
    c = min(max(int(site_prob * P) - 2, 0), P + 1)
    while c <= P and not (c / P >= site_prob):
        c += 1
    return c


def parse_min_fraction(text: str) -> Fraction:
    """--min_fraction from the flag's text, exactly (fractions.Fraction)."""
    from .cli import FlagError

    try:
        fr = Fraction(str(text).strip())
    except (ValueError, ZeroDivisionError) as e:
        raise FlagError(f"invalid value for --min_fraction: {text!r} ({e})")
    if fr < 0 or fr > 1:
        raise FlagError(f"--min_fraction must lie in [0, 1]: {text!r}")
    if fr.denominator > MAX_FRACTION_DENOMINATOR:
        raise FlagError(f"--min_fraction {text!r} has the denominator {fr.denominator}, above "
                        f"{MAX_FRACTION_DENOMINATOR}")
    return fr


def _regime_matrix(path: str):
    import pandas as pd

    d = pd.read_csv(path, sep="\t").set_index("pos")
    return d.index.to_numpy().astype(np.int64), d.to_numpy()


def chromosome_regions(chrom: str, results_dir: str, K: int, site_prob: float, max_gap: int, min_sites: int,
                       fraction: Fraction, device):
    """One chromosome's region table: (P, positions of the first and last site
    [n][2], n_sites [n], (n_all, n_frac) [n][2], column sums [n][2 + 2K]), numpy."""
    torch = _torch()
    pos, ctrl = _regime_matrix(os.path.join(results_dir, f"control_regimes_chrom_{chrom}.csv.gz"))
    _, case = _regime_matrix(os.path.join(results_dir, f"case_regimes_chrom_{chrom}.csv.gz"))
    if case.shape != ctrl.shape:
        raise ValueError(f"chromosome {chrom}: the control and case matrices differ in shape")
    T, P = ctrl.shape
    c_dev, k_dev = _upload_regimes(ctrl, device), _upload_regimes(case, device)
    m_dev = torch.ones((T, P), dtype=torch.int16, device=device)  # merged states are not an input here
    counts, _ = site_counts(m_dev, c_dev, k_dev, P, K, [(0, T)], [[0]], T)
    del m_dev
    p_dev = torch.from_numpy(np.ascontiguousarray(pos)).to(device)
    regions = find_regions(counts, 1, min_count_of(site_prob, P), p_dev, max_gap, min_sites).contiguous()
    rc = region_counts(c_dev, k_dev, P, [(0, T)], [[0]], T, regions, fraction)
    sums = region_sums(counts, regions)
    torch.cuda.synchronize(device)
    reg = regions.cpu().numpy()
    span = np.stack([pos[reg[:, 0]], pos[reg[:, 1] - 1]], 1) if len(reg) else np.zeros((0, 2), np.int64)
    return P, span, reg[:, 1] - reg[:, 0], rc.cpu().numpy(), sums.cpu().numpy()


def _rows(chrom, span, n_sites, rc, sums, P: int, K: int, mu: np.ndarray) -> List[tuple]:
    out = []
    for i in range(len(n_sites)):
        n, n_all, n_frac = int(n_sites[i]), int(rc[i, 0]), int(rc[i, 1])
        h_ctrl = [int(x) for x in sums[i, 2:2 + K]]
        h_case = [int(x) for x in sums[i, 2 + K:2 + 2 * K]]
        d = 0.0
        for r in range(K):
            d += float(mu[r]) * (h_case[r] - h_ctrl[r])
        out.append((chrom, int(span[i, 0]), int(span[i, 1]), n, n_all, n_frac, n_all / P, n_frac / P,
                    1. - n_frac / P, int(sums[i, 1]) / (n * P), d / (n * P),
                    int(np.argmax(h_ctrl)) + 1, int(np.argmax(h_case)) + 1))
    return out


def _write(path: str, rows: Sequence[tuple]) -> None:
    with open(path, "w") as fh:
        fh.write("\t".join(COLUMNS) + "\n")
        for r in rows:
            fh.write("\t".join(repr(v) if isinstance(v, float) else str(v) for v in r) + "\n")


def get_dmrs_main(argv: Sequence[str]) -> int:
    """`hygeia get_dmrs`: candidate regions of every chromosome (one chromosome's
    matrices resident at a time), pooled; FDR_procedure on the pooled
    1 - n_frac / P per threshold; dmr_candidates.tsv and dmr_{thr}.tsv."""
    import sys

    torch = _torch()
    from .cli import FlagError, parse_flags

    f = parse_flags(argv, GET_DMRS_FLAGS)
    K = int(f["n_regimes"])
    fraction = parse_min_fraction(f["min_fraction"])
    mu = np.array([float(x) for x in f["mu"]], dtype=np.float64)
    if mu.shape[0] != K:
        raise FlagError(f"--mu holds {mu.shape[0]} values, --n_regimes is {K}")
    site_prob = float(f["site_prob"])
    if not 0. <= site_prob <= 1.:
        raise FlagError("--site_prob must lie in [0, 1]")
    if int(f["min_sites"]) < 1 or int(f["max_gap_bp"]) < 0:
        raise FlagError("--min_sites must be >= 1 and --max_gap_bp >= 0")
    chroms = [c for c in str(f["chroms"]).split(",") if c != ""]
    if not chroms:
        raise FlagError("--chroms is empty")
    out_dir = f["output_dir"]
    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device("cuda", 0)
    rows, P = [], None
    for chrom in chroms:
        Pc, span, n_sites, rc, sums = chromosome_regions(chrom, f["results_dir"], K, site_prob, int(f["max_gap_bp"]),
                                                         int(f["min_sites"]), fraction, dev)
        if P is not None and Pc != P:
            print(f"hygeia get_dmrs: chromosome {chrom} has {Pc} trajectories, the chromosomes before it {P}",
                  file=sys.stderr)
            return 1
        P = Pc
        rows.extend(_rows(chrom, span, n_sites, rc, sums, P, K, mu))
    _write(os.path.join(out_dir, "dmr_candidates.tsv"), rows)
    if rows:
        n_frac = np.array([r[5] for r in rows], dtype=np.int32)
        null_stat = 1. - n_frac.astype(np.int64) / P
        pooled = torch.from_numpy(n_frac.reshape(-1, 1).copy()).to(dev)
    for thr in f["fdr_thresholds"]:
        sel = []
        if rows:
            _, _, threshold = fdr(pooled, 0, P, thr)
            sel = [r for r, t in zip(rows, null_stat) if t < threshold]
        _write(os.path.join(out_dir, "dmr_{}.tsv".format(thr)), sel)
    return 0
