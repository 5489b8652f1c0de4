"""Validation on the device (cwf/validation.py, Trainer.validate, train_no_amp.py --valid_freq, evaluate.py), model at 64^3 with
roi_size (64, 64, 64), on subjects of (80, 72, 66), (64, 64, 64) and (72, 64, 48) voxels: several windows per axis, exactly one window,
and an axis shorter than the window.

Everything compared here is an integer count or a float64 ratio of such counts, so the bound is zero wherever the forward is
reproducible from call to call; `spread` (two runs of one Validator on one model) measures whether it is, and the equalities between
tables are held to it."""
import csv
import functools
import json
import logging
import os

import numpy as np
import pytest
import torch

import predict_overlap as po
from oracle import reference_model as rm
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROI = (64, 64, 64)
SIZES = [(80, 72, 66), (64, 64, 64), (72, 64, 48)]
WINDOW = {"roi_size": ROI, "overlap": 0.5}


@functools.lru_cache(maxsize=None)
def _state():
    return syn.det_state_dict(rm.param_shapes())


def _model(dropout=False):
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    m = get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="fixed")
    m.load_state_dict(_state(), strict=False)
    if not dropout:
        m.Unet_list.InitConv.dropout = 0.0
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _eval_model():
    return _model().eval()


@functools.lru_cache(maxsize=None)
def _subjects(masked=False):
    out = []
    for i, size in enumerate(SIZES):
        x, t = syn.synthetic_volume(i, size)
        if masked:                                           # zero outside an ellipsoid, as a skull-stripped subject is
            box = (tuple(s // 8 for s in size), tuple(s - s // 6 for s in size))
            m = syn.ellipsoid_mask(size, box)
            x, t = x * m[None].to(x.dtype), t * m.to(t.dtype)
        out.append((x, t.to(torch.uint8)))
    return tuple(out)


def _validator(**kw):
    from cwf.validation import Validator
    kw.setdefault("window", WINDOW)
    subjects = _subjects(bool(kw["window"].get("crop_nonzero")))
    return Validator(list(kw.pop("subjects", subjects)), DEV, **kw)


def _table(v, model):
    ints, hd = v.fill_table(model)
    return ints.cpu()


@functools.lru_cache(maxsize=None)
def _spread():
    """largest difference of a count between two runs of one Validator on one model: 0 when the forward is reproducible"""
    v = _validator()
    a, b = _table(v, _eval_model()), _table(v, _eval_model())
    return int((a - b).abs().max()), a


def _plain_rows(subjects, window, use_tta=False, postprocess=None):
    """a plain loop of validate_softmax per case: the 19 integers counted by torch from its label map, and its Dice / IoU values"""
    rows, dice, iou = [], [], []
    for x, t in subjects:
        xd, td = x[None].to(DEV), t[None].to(DEV)
        seg, _, d, m = po.validate_softmax(xd, td, _eval_model(), deterministic=True, use_TTA=use_tta, with_miou=True, window=window,
                                           postprocess=postprocess)
        rows.append(po.label_counts(seg, td.long()).reshape(-1).tolist() + [td.numel()])
        dice.append([float(v) for v in d])
        iou.append([float(v) for v in m])
    return torch.tensor(rows, dtype=torch.int64), np.array(dice), np.array(iou)


# ------------------------------------------------------------------------------------------------ 1. the table against plain calls
def test_two_runs_of_one_validator_are_bit_equal(hip):
    spread, table = _spread()
    print("call-to-call spread of the counts: %d" % spread)
    assert spread == 0
    assert table[:, 18].tolist() == [80 * 72 * 66, 64 * 64 * 64, 72 * 64 * 48] and bool((table[:, 1] > 0).all())        # voxel counts; something was predicted


@pytest.mark.parametrize("case", ["default", "crop_nonzero", "tta", "postprocess", "uncached"])
def test_table_equals_plain_validate_softmax_calls(hip, case):
    spread = _spread()[0]
    kw = {"default": {}, "crop_nonzero": {"window": dict(WINDOW, crop_nonzero=True)}, "tta": {"use_tta": True},
          "postprocess": {"postprocess": po.REFERENCE_POSTPROCESS}, "uncached": {"cache": False}}[case]
    subjects = _subjects(case == "crop_nonzero")
    if case == "tta":
        subjects = subjects[1:]                              # eight flips each: the one-window and the short-axis subject
        kw["subjects"] = subjects
    v = _validator(**kw)
    assert (v._cached is None) == (case == "uncached")
    res = v.run(_eval_model())
    want, dice, iou = _plain_rows(subjects, v.window, kw.get("use_tta", False), kw.get("postprocess"))
    got = torch.from_numpy(np.concatenate([res.counts.reshape(len(res), 18), res.voxels[:, None]], axis=1))
    print("%s: largest count difference %d (spread %d)" % (case, int((got - want).abs().max()), spread))
    assert int((got - want).abs().max()) <= spread
    if spread == 0:
        assert res.dice.tobytes() == dice.tobytes() and res.iou.tobytes() == iou.tobytes()          # bit for bit
    if case == "crop_nonzero":
        plain = _table(_validator(subjects=subjects), _eval_model())
        assert not torch.equal(plain, got)                   # the cropped windows are other windows: the setting took effect


def test_hd95_column_equals_plain_calls(hip):
    subjects = _subjects()[1:]
    res = _validator(subjects=subjects, with_hd95=True).run(_eval_model())
    for i, (x, t) in enumerate(subjects):
        out = po.validate_softmax(x[None].to(DEV), t[None].to(DEV), _eval_model(), with_hd95=True, window=WINDOW)
        if _spread()[0] == 0:
            assert res.hd95[i].tolist() == out[3][0].tolist()
    assert res.mean_hd95.shape == (3,) and "hd95_wt" in res.to_rows()[0]


# ------------------------------------------------------------------------------------------------ 2. shards
def test_two_shards_sum_to_the_one_rank_table(hip):
    spread, full = _spread()
    parts = [_table(_validator(rank=r, world=2), _eval_model()) for r in (0, 1)]
    assert not parts[0][1].any() and not parts[1][0].any() and not parts[1][2].any()
    assert int((parts[0] + parts[1] - full).abs().max()) <= spread


# ------------------------------------------------------------------------------------------------ 3. Trainer.validate leaves no trace
def _reset_rng(hip, seed=1000):
    torch.manual_seed(seed)
    hip.rng(torch.device(DEV)).copy_(torch.tensor([seed, 0], dtype=torch.int64))


def _batch(i):
    return tuple(t.to(DEV) for t in syn.synthetic_batch([i], ROI))


def _snapshot(tr, hip):
    tr.opt._ensure()
    tensors = [p.detach().clone() for p in tr.model.parameters()] + [b.detach().clone() for b in tr.model.buffers()]
    for p in tr.opt._plist:
        tensors += [v.detach().clone() for v in tr.opt.state[p].values() if torch.is_tensor(v)]
    tensors += [e.clone() for e in (tr.opt.ema or [])]
    tensors.append(hip.rng(torch.device(DEV)).clone())
    return tensors, [m.training for m in tr.model.modules()], tr.model.Unet_list.InitConv.dropout


@pytest.mark.parametrize("mode", ["eager", "plan"])
def test_trainer_validate_leaves_no_trace(hip, mode):
    from cwf.trainer import Trainer
    _reset_rng(hip)
    tr = Trainer(_model(dropout=True).train(), use_graph="plan" if mode == "plan" else False, graph_warmup=2, ema_decay=0.9)
    assert tr.model.Unet_list.InitConv.dropout > 0.0
    for i in range(3):
        tr.step(*_batch(i), 0)
    assert (tr._plan is not None) == (mode == "plan"), tr.plan_info       # validation after the capture
    static = tr.static_inputs
    v = _validator(subjects=_subjects()[1:])
    for use_ema in (False, True):
        before, modes, dropout = _snapshot(tr, hip)
        res = tr.validate(v, use_ema=use_ema)
        after, modes2, dropout2 = _snapshot(tr, hip)
        assert len(res) == 2 and np.isfinite(res.score)
        assert all(torch.equal(a, b) for a, b in zip(before, after)) and len(before) == len(after)
        assert modes == modes2 and all(modes) and dropout == dropout2
        assert tr.static_inputs is static and tr._micro == 0
    loss, parts = tr.step(*_batch(3), 0)
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p)) for p in parts)


# ------------------------------------------------------------------------------------------------ 4. the training trajectory
def _four_steps(hip, validate_after=None):
    from cwf.trainer import Trainer
    _reset_rng(hip)
    tr = Trainer(_model(dropout=True).train())
    for i in range(4):
        tr.step(*_batch(i), 0)
        if validate_after == i:
            tr.validate(_validator(subjects=_subjects()[1:2]))
    torch.cuda.synchronize()
    return torch.cat([p.detach().reshape(-1) for p in tr.model.parameters()])


def test_validation_does_not_move_the_training_trajectory(hip, monkeypatch):
    """Measured on an MI355X (one run of this test): the two plain runs are bit-equal in every weight, so the validated run is held to
    bit equality."""
    from cwf.trainer import Trainer
    plain = [_four_steps(hip), _four_steps(hip)]
    noise = float((plain[0] - plain[1]).abs().max())
    validated = _four_steps(hip, validate_after=1)
    diff = float((validated - plain[0]).abs().max())
    print("plain against plain: %.3e, validated against plain: %.3e" % (noise, diff))
    assert diff <= 4 * noise                                 # bit-equal when the plain runs are; else 4 x their spread
    monkeypatch.setattr(Trainer, "_restore_rng", staticmethod(lambda rng, saved: None))
    unrestored = _four_steps(hip, validate_after=1)
    control = float((unrestored - plain[0]).abs().max())
    print("control, generator words left unrestored: %.3e" % control)
    assert control > 0.0 and control > 4 * noise             # the assertion above can fail


# ------------------------------------------------------------------------------------------------ 5. EMA
def test_validate_use_ema_scores_the_ema_weights(hip):
    from cwf.trainer import Trainer
    _reset_rng(hip)
    tr = Trainer(_model().train(), lr=1e-3, ema_decay=0.5)
    for i in range(3):
        tr.step(*_batch(i), 0)
    v = _validator(subjects=_subjects()[1:])
    raw_before = [p.detach().clone() for p in tr.model.parameters()]
    ptrs = [p.data_ptr() for p in tr.model.parameters()]
    ema_before = [e.clone() for e in tr.opt.ema]
    ema_table = tr.validate(v, use_ema=True)
    assert all(torch.equal(a, p.detach()) for a, p in zip(raw_before, tr.model.parameters()))
    assert ptrs == [p.data_ptr() for p in tr.model.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(ema_before, tr.opt.ema))
    raw_table = tr.validate(v)
    fresh = _model()
    fresh.load_state_dict(tr.ema_state_dict())
    fresh_table = v.run(fresh.eval())
    spread = _spread()[0]
    assert int(np.abs(ema_table.counts - fresh_table.counts).max()) <= spread
    assert int(np.abs(ema_table.counts - raw_table.counts).max()) > spread


# ------------------------------------------------------------------------------------------------ 6. errors
def test_validate_errors(hip):
    from cwf.trainer import Trainer
    v = _validator(subjects=_subjects()[1:2])
    tr = Trainer(_model().train(), accum_steps=2)
    with pytest.raises(RuntimeError, match="no EMA"):
        tr.validate(v, use_ema=True)
    tr.step(*_batch(0), 0)
    with pytest.raises(ValueError, match="accumulation window"):
        tr.validate(v)
    tr.step(*_batch(1), 0)
    assert len(tr.validate(v)) == 1


# ------------------------------------------------------------------------------------------------ 7. end to end
@pytest.fixture()
def fresh_train_log():
    """train_no_amp attaches its log handlers once per process: drop the ones this test adds; and put the precision back"""
    from cwf import kernels
    log = logging.getLogger("cwf.train")
    before, precision = list(log.handlers), kernels.precision()
    yield
    kernels.set_precision(precision)
    for h in list(log.handlers):
        if h not in before:
            log.removeHandler(h)
            h.close()


@pytest.mark.parametrize("step_mode", ["eager", "plan"])
def test_train_validate_and_evaluate_end_to_end(hip, fresh_train_log, tmp_path, caplog, step_mode):
    import evaluate
    import train_no_amp as tn
    from cwf.trainer import load_checkpoint
    root = str(tmp_path)
    shape = ["--input_H", "72", "--input_W", "64", "--output_D", "66", "--crop_H", "64", "--crop_W", "64", "--crop_D", "64"]
    with caplog.at_level(logging.INFO, logger="cwf.train"):
        assert tn.main(["--synthetic", "2", "--valid_synthetic", "2", "--valid_freq", "1", "--end_epoch", "2", "--num_workers", "0",
                        "--project_root", root, "--experiment", "e", "--date", "d", "--log_every", "1", "--step_mode", step_mode,
                        "--save_freq", "1000"] + shape) == 0
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Validation: epoch")]
    assert len(lines) == 2 and lines[1].startswith("Validation: epoch 1 ") and "score" in lines[1]
    records = json.load(open(os.path.join(root, "log", "ed_valid.json")))
    assert [r["epoch"] for r in records] == [0, 1] and records[0]["is_best"] and all(r["cases"] == 2 for r in records)
    best = max(records, key=lambda r: r["score"])
    assert records[-1]["best_epoch"] == (0 if records[0]["score"] >= records[1]["score"] else 1) and records[-1]["best_score"] == best["score"]
    ck = os.path.join(root, "checkpoint", "ed")
    assert load_checkpoint(os.path.join(ck, "model_best.pth"), _model()) == records[-1]["best_epoch"]
    out = os.path.join(root, "eval")
    assert evaluate.main(["--resume", os.path.join(ck, "model_epoch_last.pth"), "--synthetic", "2", "--synthetic_first", "2", "--out", out,
                          "--save_seg", "true", "--cache", "true"] + shape) == 0
    rows = list(csv.DictReader(open(os.path.join(out, "cases.csv"))))
    assert [r["name"] for r in rows] == records[-1]["names"]
    got = [[float(r["dice_" + k]) for k in ("wt", "tc", "et")] for r in rows]
    if _spread()[0] == 0:
        assert got == records[-1]["case_dice"]
        assert json.load(open(os.path.join(out, "summary.json")))["score"] == records[-1]["score"]
    for r in rows:
        seg = np.load(os.path.join(out, r["name"] + ".npy"))
        assert seg.dtype == np.uint8 and seg.shape == (72, 64, 66) and set(np.unique(seg).tolist()) <= {0, 1, 2, 4}
        assert int((seg > 0).sum()) == int(r["pred_wt"])
