"""Validation on the device: ``Validator`` runs predict_overlap.validate_softmax over a list of whole subjects and gathers one row of
integer counts per case in a device table; ``ValidationResult`` turns the table into the numbers people report.

The loop.  Per case: the subject (cached on the device, or loaded when its turn comes), validate_softmax(deterministic=True,
with_counts=True) with the window / TTA / post-processing settings, and the case's row written by device copies: the [6][3] int64 counts
(|o & t|, |o|, |t|) of WT, TC, ET, class 1, 2, 3 that cwf_argmax_metrics / cwf_label_metrics left on the device, the voxel count, and
with ``with_hd95`` the three HD95 values in a float64 table beside it.  Nothing is read back inside the loop (except the nonzero box
that "crop_nonzero" reads back for its windows); one copy to the host ends the run.

Sharding.  Rank r of `world` takes the cases i with i % world == r (shard_cases): no padding, no case twice -- cwf.parallel.shard_indices
pads to equal length, as a DistributedSampler does, which would count some cases twice.  Rows of other ranks stay zero, and with
world > 1 one all_reduce(SUM) of the integer table (and one of the float table, when there is one) follows the loop: zero plus a value
is that value, exactly, in int64 and in float64, so every rank then holds the table a single rank would have filled, and every
aggregate, taken from the reduced table on the host, is the same bit for bit at any world size.

Aggregates (ValidationResult, numpy float64, case order).  Per case: Dice (2 |o & t| + 1e-8) / (|o| + |t| + 1e-8) of WT / TC / ET and
IoU (|o & t| + 1e-8) / (|o| + |t| - |o & t| + 1e-8) of classes 1..3, the formulas of argmax_dice, so a region empty in both maps scores
1, one empty in one map only scores 1e-8 / (n + 1e-8), about 0.  Over the cases: mean, population standard deviation, median and
quartiles (linear interpolation) of each; the global Dice, same formula on the counts summed over cases (nnU-Net's); sensitivity
|o & t| / |t|, precision |o & t| / |o| and specificity (V - |o| - |t| + |o & t|) / (V - |t|) of WT / TC / ET from the summed counts and
the summed voxel count V, NaN where the denominator is 0; `score`, the mean of the three mean Dice values.  No case: every aggregate
is NaN."""
import json
import math
import os

import numpy as np
import torch
import torch.distributed as dist

REGIONS = ("wt", "tc", "et")
CLASSES = ("1", "2", "3")
COUNT_NAMES = tuple("%s_%s" % (kind, r) for r in REGIONS + tuple("c" + c for c in CLASSES) for kind in ("both", "pred", "target"))
INT_COLUMNS = 19                    # 18 counts and the voxel count
DEFAULT_WINDOW = {"roi_size": (128, 128, 128), "overlap": 0.5}


def shard_cases(n_cases, rank, world):
    """The cases of rank `rank` of `world`, in subject order: i with i % world == rank."""
    if int(world) < 1 or not 0 <= int(rank) < int(world):
        raise ValueError("shard_cases: need world >= 1 and 0 <= rank < world, got rank %r of %r" % (rank, world))
    return list(range(int(rank), int(n_cases), int(world)))


def better_score(score, best):
    """True when `score` takes the place of `best` (None: nothing so far): strictly greater.  A tie keeps the earlier one, a NaN never
    wins, and a NaN that somehow holds the place loses to any number."""
    if score is None or math.isnan(score):
        return False
    return best is None or math.isnan(best) or score > best


def _ratio(num, den):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.full(num.shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def _spread(v):
    """mean, population std, median and quartiles of the columns of v [N, K] -> dict of [K] arrays (NaN when N = 0)"""
    if v.shape[0] == 0:
        nan = np.full(v.shape[1], np.nan)
        return {k: nan.copy() for k in ("mean", "std", "median", "q1", "q3")}
    q1, med, q3 = np.percentile(v, [25.0, 50.0, 75.0], axis=0)
    return {"mean": v.mean(axis=0), "std": v.std(axis=0), "median": med, "q1": q1, "q3": q3}


class ValidationResult:
    """What a (reduced) validation table says.  `ints` [N, 19] int64: per case the 18 counts (COUNT_NAMES order, i.e. [6][3] flattened)
    and the voxel count; `hd95` None or [N, 3] float64; `names` one string per case.  Attributes, all numpy float64 in case order unless
    said otherwise: counts [N, 6, 3] int64, voxels [N] int64, dice [N, 3], iou [N, 3], dice_stats / iou_stats (dicts of mean, std,
    median, q1, q3, each [3]), global_dice [3], sensitivity / specificity / precision [3], score (float), hd95 and mean_hd95 [3] or
    None."""

    def __init__(self, ints, hd95=None, names=None):
        ints = np.ascontiguousarray(np.asarray(ints, dtype=np.int64)).reshape(-1, INT_COLUMNS)
        n = ints.shape[0]
        self.names = ["case_%04d" % i for i in range(n)] if names is None else list(names)
        if len(self.names) != n:
            raise ValueError("ValidationResult: %d names for %d cases" % (len(self.names), n))
        self.counts, self.voxels = ints[:, :18].reshape(n, 6, 3), ints[:, 18]
        c = self.counts.astype(np.float64)
        self.dice = (2 * c[:, :3, 0] + 1e-8) / (c[:, :3, 1] + c[:, :3, 2] + 1e-8)
        self.iou = (c[:, 3:, 0] + 1e-8) / (c[:, 3:, 1] + c[:, 3:, 2] - c[:, 3:, 0] + 1e-8)
        self.dice_stats, self.iou_stats = _spread(self.dice), _spread(self.iou)
        if n:
            g = self.counts[:, :3].sum(axis=0).astype(np.float64)          # summed in int64: exact
            vox = float(self.voxels.sum())
            self.global_dice = (2 * g[:, 0] + 1e-8) / (g[:, 1] + g[:, 2] + 1e-8)
            self.sensitivity, self.precision = _ratio(g[:, 0], g[:, 2]), _ratio(g[:, 0], g[:, 1])
            self.specificity = _ratio(vox - g[:, 1] - g[:, 2] + g[:, 0], vox - g[:, 2])
        else:
            self.global_dice, self.sensitivity, self.precision, self.specificity = (np.full(3, np.nan) for _ in range(4))
        self.score = float(self.dice_stats["mean"].mean())
        self.hd95 = None if hd95 is None else np.asarray(hd95, dtype=np.float64).reshape(n, 3)
        self.mean_hd95 = None if self.hd95 is None else (self.hd95.mean(axis=0) if n else np.full(3, np.nan))

    def __len__(self):
        return len(self.names)

    def to_rows(self):
        """One dict per case, in case order: name, dice_wt/tc/et, iou_1/2/3, the 18 counts under COUNT_NAMES, voxels and, when there,
        hd95_wt/tc/et.  Values are Python floats and ints."""
        rows = []
        for i, name in enumerate(self.names):
            row = {"name": name}
            row.update(("dice_" + r, float(self.dice[i, k])) for k, r in enumerate(REGIONS))
            row.update(("iou_" + c, float(self.iou[i, k])) for k, c in enumerate(CLASSES))
            row.update((cn, int(v)) for cn, v in zip(COUNT_NAMES, self.counts[i].reshape(-1)))
            row["voxels"] = int(self.voxels[i])
            if self.hd95 is not None:
                row.update(("hd95_" + r, float(self.hd95[i, k])) for k, r in enumerate(REGIONS))
            rows.append(row)
        return rows

    def to_json(self):
        """The aggregates and the per-case Dice / IoU as a dict of plain Python values (json.dumps takes it; NaN stays NaN)."""
        lst = lambda a: [float(v) for v in a]
        out = {"cases": len(self), "score": self.score, "names": list(self.names),
               "dice": {k: lst(v) for k, v in self.dice_stats.items()}, "iou": {k: lst(v) for k, v in self.iou_stats.items()},
               "global_dice": lst(self.global_dice), "sensitivity": lst(self.sensitivity), "specificity": lst(self.specificity),
               "precision": lst(self.precision), "case_dice": [lst(r) for r in self.dice], "case_iou": [lst(r) for r in self.iou]}
        if self.hd95 is not None:
            out["mean_hd95"], out["case_hd95"] = lst(self.mean_hd95), [lst(r) for r in self.hd95]
        return out


class Validator:
    """Whole-subject validation with one device table per run (see the module text).

    subjects: what utils.data.NpzCropSource takes -- .npz paths, or in-memory (image [4,S0,S1,S2] float32, label uint8) pairs; whole
    volumes of any extents, differing between cases.  Label 4 is read as 3.  cache=True holds them on `device` (fp32 image, uint8
    label) from construction on -- only this rank's cases; cache=False loads each case when its turn comes.  normalize applies
    utils.data.normalize_nonzero.
    window: a dict of sliding_window_inference keywords (DEFAULT_WINDOW when None; "crop_nonzero": True is allowed); use_tta and
    postprocess as validate_softmax's use_TTA and postprocess.  with_hd95 adds the three HD95 values per case (device only).
    rank / world: the shard (shard_cases); with world > 1 run() ends with the all_reduce of the table over the default process
    group, so every rank must call it.
    predict: a callable x [1,4,...] -> probabilities [1,4,...] that stands in for the model and the windows (validate_softmax's
    predict); with it `device` may be the CPU, where the counts come from torch reductions."""

    def __init__(self, subjects, device, *, window=None, use_tta=False, postprocess=None, normalize=False, cache=True, with_hd95=False,
                 rank=0, world=1, predict=None):
        from utils.data import NpzCropSource
        self.device = torch.device(device)
        if self.device.type != "cuda" and predict is None:
            raise ValueError("Validator: the model predicts on the device only; on %s give predict=" % self.device)
        if self.device.type != "cuda" and with_hd95:
            raise ValueError("Validator: with_hd95 runs on the device kernels only")
        self.window = dict(DEFAULT_WINDOW) if window is None else dict(window)
        self.use_tta, self.postprocess, self.with_hd95, self.predict = bool(use_tta), postprocess, bool(with_hd95), predict
        self.rank, self.world = int(rank), int(world)
        self.normalize = bool(normalize)                # on the device by its kernel, as DeviceBraTS does; on the CPU by the source
        self.source = NpzCropSource(subjects, self.window.get("roi_size", DEFAULT_WINDOW["roi_size"]),
                                    normalize=self.normalize and self.device.type != "cuda")
        self.names = [os.path.splitext(os.path.basename(s))[0] if isinstance(s, str) else "case_%04d" % i
                      for i, s in enumerate(self.source.subjects)]
        self.mine = shard_cases(len(self.source), self.rank, self.world)
        self._cached = {i: self._load(i) for i in self.mine} if cache else None

    def __len__(self):
        return len(self.source)

    def _load(self, i):
        """subject i as (x [1,4,S0,S1,S2] float32, target [1,S0,S1,S2] uint8 with label 4 read as 3) on the device"""
        from utils.data import normalize_nonzero
        img, lab = self.source.load(i)
        lab = torch.where(lab == 4, torch.full_like(lab, 3), lab)
        img, lab = img.to(self.device).contiguous(), lab.to(self.device).contiguous()
        if self.normalize and img.is_cuda:              # (on the CPU the source has normalised its own copy)
            normalize_nonzero(img)
        return img[None], lab[None]

    def case(self, i):
        return self._cached[i] if self._cached is not None else self._load(i)

    def fill_table(self, model=None, on_case=None):
        """This rank's rows: (ints [N, 19] int64, hd95 [N, 3] float64 or None) on the device, rows of other ranks zero, nothing
        reduced and nothing read back.  on_case as in run."""
        import predict_overlap as po
        n = len(self)
        ints = torch.zeros((n, INT_COLUMNS), dtype=torch.int64, device=self.device)
        hd = torch.zeros((n, 3), dtype=torch.float64, device=self.device) if self.with_hd95 else None
        for i in self.mine:
            x, target = self.case(i)
            res = po.validate_softmax(x, target, model, deterministic=True, use_TTA=self.use_tta, with_hd95=self.with_hd95,
                                      window=self.window, postprocess=self.postprocess, with_counts=True, predict=self.predict)
            ints[i, :18] = res[-1].reshape(-1)
            ints[i, 18] = target.numel()
            if hd is not None:
                hd[i] = res[3][0]
            if on_case is not None:
                on_case(i, res[0], target, res[1])
        return ints, hd

    def result_of(self, ints, hd=None):
        """The ValidationResult of (reduced) device tables: one copy to the host (the float table's bits ride behind the integer
        columns)."""
        if hd is None:
            return ValidationResult(ints.cpu().numpy(), None, self.names)
        host = torch.cat([ints, hd.view(torch.int64)], dim=1).cpu()
        return ValidationResult(host[:, :INT_COLUMNS].numpy(), host[:, INT_COLUMNS:].contiguous().view(torch.float64).numpy(), self.names)

    def run(self, model=None, on_case=None):
        """Fill the table, reduce it over the ranks, copy it to the host once and return its ValidationResult.  on_case(i, seg, target,
        prob): called after case i of this rank's shard with its final label map (int64 [1,S0,S1,S2]), target (uint8) and
        probabilities -- for writers and per-case metrics outside the table; what it reads back is its own affair."""
        ints, hd = self.fill_table(model, on_case)
        if self.world > 1:
            dist.all_reduce(ints, op=dist.ReduceOp.SUM)
            if hd is not None:
                dist.all_reduce(hd, op=dist.ReduceOp.SUM)
        return self.result_of(ints, hd)


def write_cases_csv(path, rows):
    """rows (ValidationResult.to_rows(), possibly with further columns) as a CSV file; floats are written with repr, so reading them
    back gives the same float64."""
    import csv
    cols = list(rows[0]) if rows else ["name"]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(cols)
        for r in rows:
            w.writerow([repr(r[c]) if isinstance(r[c], float) else r[c] for c in cols])


def write_json(path, obj):
    """obj as JSON, written whole through a temporary file beside it"""
    tmp = path + ".tmp"
    with open(tmp, "w") as f:
        json.dump(obj, f, indent=1)
    os.replace(tmp, path)
