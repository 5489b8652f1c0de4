"""CPU: cwf.validation -- the aggregates against tests/validation_ref.py, the sharding rule, the table of Validator(predict=...) on CPU
tensors, a gloo world-2 run, the best-score rule, and train_no_amp.py's argument errors and its unchanged files with validation off.

Tolerances.  Per-case Dice / IoU, the global Dice and the three rates are single expressions of integers: compared exactly.  Mean,
standard deviation, quartiles and the score are sums over N <= 8 values in [0, 1] that numpy and the restatement add in different
orders and interpolate by different but equivalent expressions: each is held to 4 N eps (eps = 2^-52), the bound of a reordered sum of
N such terms with room for the square root and the interpolation."""
import glob
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import validation_ref as vr

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd")
EPS = 2.0 ** -52


def row(wt, tc, et, c1, c2, c3, vox):
    return list(wt) + list(tc) + list(et) + list(c1) + list(c2) + list(c3) + [vox]


# (|o & t|, |o|, |t|) per region; the cases hold: a region empty in both maps (ET of case 0, class 3 too), one empty in the target only
# (TC of case 1), one empty in the prediction only (ET of case 2), and plain ones
TABLE = [row((90, 100, 120), (40, 50, 45), (0, 0, 0), (40, 50, 45), (50, 50, 75), (0, 0, 0), 1000),
         row((10, 30, 10), (0, 7, 0), (0, 3, 0), (0, 4, 0), (10, 23, 10), (0, 3, 0), 512),
         row((300, 310, 400), (100, 120, 200), (0, 0, 60), (100, 120, 140), (150, 190, 200), (0, 0, 60), 4096),
         row((5, 5, 5), (2, 2, 2), (1, 1, 1), (1, 1, 1), (3, 3, 3), (1, 1, 1), 64)]


def check_against_ref(table):
    from cwf.validation import ValidationResult
    res, ref = ValidationResult(np.array(table, dtype=np.int64).reshape(-1, 19)), vr.aggregates(table)
    n = len(res)
    assert np.array_equal(res.dice, ref["dice"]) and np.array_equal(res.iou, ref["iou"])
    for name in ("global_dice", "sensitivity", "specificity", "precision"):
        assert np.array_equal(getattr(res, name), ref[name], equal_nan=True), name
    tol = 4 * max(n, 1) * EPS
    for got, want in ((res.dice_stats, ref["dice_stats"]), (res.iou_stats, ref["iou_stats"])):
        for key in ("mean", "std", "median", "q1", "q3"):
            for r in range(3):
                g, w = got[key][r], want[r][key]
                assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= tol, (key, r, g, w)
    assert (math.isnan(res.score) and math.isnan(ref["score"])) or abs(res.score - ref["score"]) <= tol
    return res


def test_result_matches_the_numpy_statement():
    res = check_against_ref(TABLE)
    assert res.dice[0, 2] == 1.0 and res.iou[0, 2] == 1.0                 # empty in both maps scores 1
    assert 0.0 < res.dice[1, 1] < 1e-8 and 0.0 < res.dice[2, 2] < 1e-8      # empty in one map only: 1e-8 / (n + 1e-8)
    assert res.score == float(np.mean(res.dice_stats["mean"]))
    rows, js = res.to_rows(), res.to_json()
    assert [r["name"] for r in rows] == res.names and rows[2]["both_wt"] == 300 and rows[2]["target_c3"] == 60 and rows[1]["voxels"] == 512
    assert js["case_dice"][3] == [1.0, 1.0, 1.0] and js["score"] == res.score and js["cases"] == 4


def test_result_single_case_and_no_case():
    res = check_against_ref(TABLE[2:3])
    assert np.array_equal(res.dice_stats["std"], np.zeros(3)) and np.array_equal(res.dice_stats["median"], res.dice[0])
    assert np.array_equal(res.dice_stats["q1"], res.dice[0]) and np.array_equal(res.global_dice, res.dice[0])
    assert math.isnan(res.precision[2]) and res.sensitivity[2] == 0.0          # nothing predicted: 0 / 0 and 0 / 60
    empty = check_against_ref([])
    assert len(empty) == 0 and math.isnan(empty.score) and empty.to_rows() == []


def _subjects(sizes, seed=7):
    from utils import synthetic as syn
    out = []
    for i, size in enumerate(sizes):
        x, t = syn.synthetic_volume(i, size, seed)
        t = t.to(torch.uint8)
        t[t == 3] = 4                                                     # BraTS files say 4: the Validator reads it as 3
        out.append((x, t))
    return out


def predictor(x):
    """a fixed map x [1,4,...] -> probabilities [1,4,...] that tracks the synthetic labels loosely (channel offsets of synthetic_volume)"""
    logits = torch.stack([0.3 + 0.0 * x[:, 0], x[:, 0] - 0.4, 0.6 * x[:, 2] - x[:, 1], x[:, 3] + 0.5 * x[:, 0] - 0.9], dim=1)
    return torch.softmax(logits, dim=1)


def test_shards_are_disjoint_cover_and_sum_to_the_one_rank_table():
    from cwf.validation import Validator, ValidationResult, shard_cases
    sizes = [(6 + i, 5, 7) for i in range(7)]
    subjects = _subjects(sizes)
    for n in range(0, 8):
        one = Validator(subjects[:n], "cpu", predict=predictor)
        full, _ = one.fill_table()
        want = one.result_of(full)
        for world in range(1, 5):
            shards = [shard_cases(n, r, world) for r in range(world)]
            assert sorted(i for s in shards for i in s) == list(range(n))                   # disjoint and covering
            assert all(s == sorted(s) and all(i % world == r for i in s) for r, s in enumerate(shards))
            total = torch.zeros_like(full)
            for r in range(world):
                v = Validator(subjects[:n], "cpu", predict=predictor, rank=r, world=world)
                assert v.mine == shards[r]
                part, _ = v.fill_table()
                others = [i for i in range(n) if i % world != r]
                assert not part[others].any()                                             # rows of other ranks stay zero
                total += part
            assert torch.equal(total, full)
            got = ValidationResult(total.numpy(), None, one.names)
            assert got.score == want.score or (math.isnan(got.score) and math.isnan(want.score))
            for a, b in zip((got.dice, got.global_dice, got.dice_stats["mean"], got.dice_stats["std"], got.iou_stats["q3"], got.specificity),
                            (want.dice, want.global_dice, want.dice_stats["mean"], want.dice_stats["std"], want.iou_stats["q3"], want.specificity)):
                assert a.tobytes() == b.tobytes()                                           # bit-equal aggregates
    with pytest.raises(ValueError):
        shard_cases(3, 2, 2)


def test_validator_counts_on_cpu_tensors_equal_numpy_counts():
    from cwf.validation import Validator
    from utils import tools
    sizes = [(12, 9, 10), (8, 8, 8), (7, 13, 6)]
    subjects = _subjects(sizes)
    before = [(x.clone(), t.clone()) for x, t in subjects]
    v = Validator(subjects, "cpu", predict=predictor)
    res = v.run()
    assert all(torch.equal(x, bx) and torch.equal(t, bt) for (x, t), (bx, bt) in zip(subjects, before))       # inputs untouched
    for i, (x, t) in enumerate(subjects):
        seg = predictor(x[None]).argmax(1)[0].numpy()
        tgt = t.numpy().astype(np.int64)
        tgt[tgt == 4] = 3
        assert res.counts[i].reshape(-1).tolist() + [int(res.voxels[i])] == vr.label_table_row(seg, tgt)
        dice = [float(d) for d in tools.softmax_output_dice(seg, tgt)]              # numpy inputs: float64, the reference's expression
        iou = [float(d) for d in tools.softmax_mIOU_score(seg, tgt)]
        assert res.dice[i].tolist() == dice and res.iou[i].tolist() == iou
        assert res.counts[i, 2, 2] > 0                                            # label 4 was read as class 3
    assert res.names == ["case_0000", "case_0001", "case_0002"]
    # TTA and post-processing go through validate_softmax's own paths
    import predict_overlap as po
    tta = Validator(subjects, "cpu", predict=predictor, use_tta=True).run()
    x, t = subjects[0]
    seg = po.flip_tta(x[None], None, lambda xb, mm: predictor(xb), batch=1).argmax(1)[0].numpy()
    tgt = t.numpy().astype(np.int64); tgt[tgt == 4] = 3
    assert tta.counts[0].reshape(-1).tolist() + [int(tta.voxels[0])] == vr.label_table_row(seg, tgt)
    pp = Validator(subjects, "cpu", predict=predictor, postprocess=dict(et_min_voxels=10 ** 6, et_replace=1)).run()
    assert int(pp.counts[:, 2, 1].sum()) == 0 and int(res.counts[:, 2, 1].sum()) > 0    # every predicted ET voxel relabelled
    with pytest.raises(ValueError):
        Validator(subjects, "cpu")                                               # the model predicts on the device only


def test_validate_softmax_defaults_are_unchanged_by_the_new_keywords():
    import predict_overlap as po
    x, t = _subjects([(9, 8, 7)])[0]
    t = torch.where(t == 4, torch.full_like(t, 3), t)
    res = po.validate_softmax(x[None], t[None], None, predict=predictor, with_miou=True)
    assert len(res) == 4
    more = po.validate_softmax(x[None], t[None], None, predict=predictor, with_miou=True, with_counts=True)
    assert len(more) == 5 and torch.equal(more[0], res[0]) and more[4].dtype == torch.int64 and tuple(more[4].shape) == (6, 3)
    assert po.validate_softmax(x[None], None, None, predict=predictor, with_counts=True)[-1] is None


def _gloo_worker(rank, world, port, ret):
    for p in (PKG, REPO, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cwf.validation import Validator
        subjects = _subjects([(10, 9, 8), (8, 8, 8), (7, 11, 6)])
        calls = []

        def counted(x):
            calls.append(tuple(x.shape))
            return predictor(x)
        res = Validator(subjects, "cpu", predict=counted, rank=rank, world=world).run()
        assert len(calls) == (2 if rank == 0 else 1)                           # cases 0, 2 and case 1: no case twice
        one = Validator(subjects, "cpu", predict=predictor).run()
        assert np.array_equal(res.counts, one.counts) and np.array_equal(res.voxels, one.voxels)
        assert res.dice.tobytes() == one.dice.tobytes() and res.score == one.score
        ret[rank] = res.counts.tobytes()
    finally:
        dist.destroy_process_group()


def test_validator_world2_gloo_every_rank_holds_the_full_table():
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 33500 + (os.getpid() % 2000)
    mp.spawn(_gloo_worker, args=(world, port, ret), nprocs=world, join=True)
    assert ret.get(0) is not None and ret.get(0) == ret.get(1)


def test_best_score_rule():
    from cwf.validation import better_score
    nan = float("nan")
    assert better_score(0.5, None) and better_score(0.6, 0.5)
    assert not better_score(0.5, 0.5)                                             # a tie keeps the earlier file
    assert not better_score(0.4, 0.5)
    assert not better_score(nan, None) and not better_score(nan, 0.1) and not better_score(nan, nan)      # a NaN never wins
    assert better_score(0.0, nan)
    best, kept = None, []
    for epoch, s in enumerate([0.2, nan, 0.2, 0.3, 0.3, 0.1]):
        if better_score(s, best):
            best = s
            kept.append(epoch)
    assert kept == [0, 3]


@pytest.fixture()
def no_model(monkeypatch):
    """fail the test if a model is built"""
    import models.clswiseformer.cls_wise_former as cwf_model
    built = []
    monkeypatch.setattr(cwf_model, "get_cls_wise_former", lambda *a, **k: built.append(1) or (_ for _ in ()).throw(AssertionError("model built")))
    return built


BASE = ["--synthetic", "1", "--crop_H", "64", "--crop_W", "64", "--crop_D", "64", "--end_epoch", "1", "--no_cuda", "true"]


@pytest.mark.parametrize("flags, message", [
    (["--valid_freq", "-1"], "--valid_freq takes"),
    (["--valid_freq", "1", "--valid_synthetic", "1", "--valid_ema", "true"], "--valid_ema .* needs --ema_decay"),
    (["--valid_freq", "1"], "found no validation subjects"),
    (["--valid_freq", "1", "--valid_synthetic", "0"], "found no validation subjects"),
    (["--valid_overlap", "0.25"], "--valid_overlap belongs to --valid_freq"),
    (["--valid_synthetic", "2"], "--valid_synthetic belongs to --valid_freq"),
    (["--valid_tta", "true", "--valid_hd95", "false"], "--valid_tta / --valid_hd95 belong to --valid_freq"),
    (["--valid_crop_nonzero", "true"], "belongs to --valid_freq"),
    (["--valid_ema", "true", "--ema_decay", "0.9"], "belongs to --valid_freq"),
    (["--valid_postprocess", "reference"], "belongs to --valid_freq"),
    (["--valid_cache", "false"], "belongs to --valid_freq"),
    (["--valid_freq", "1", "--valid_synthetic", "1", "--valid_overlap", "1.0"], "--valid_overlap takes"),
    (["--valid_freq", "1", "--valid_synthetic", "1"], "device kernels only"),          # (--no_cuda true in BASE)
])
def test_argument_errors_exit_before_a_model_is_built(no_model, tmp_path, flags, message):
    import train_no_amp as tn
    with pytest.raises(SystemExit, match=message):
        tn.main(BASE + ["--project_root", str(tmp_path / "p"), "--root", str(tmp_path)] + flags)
    assert no_model == [] and not os.path.exists(tmp_path / "p")


def test_training_without_valid_freq_writes_the_files_it_wrote_before(emul_backend, tmp_path):
    import logging
    import train_no_amp as tn
    log = logging.getLogger("cwf.train")
    for h in list(log.handlers):
        log.removeHandler(h); h.close()
    try:
        rc = tn.main(["--synthetic", "2", "--crop_H", "64", "--crop_W", "64", "--crop_D", "64", "--end_epoch", "1", "--max_iters", "1",
                      "--project_root", str(tmp_path), "--experiment", "t", "--date", "d", "--no_cuda", "true"])
    finally:
        for h in list(log.handlers):
            log.removeHandler(h); h.close()
    assert rc == 0
    files = sorted(os.path.relpath(p, tmp_path) for p in glob.glob(str(tmp_path / "**" / "*"), recursive=True) if os.path.isfile(p))
    assert files == [os.path.join("checkpoint", "td", "model_epoch_last.pth"), os.path.join("log", "td.txt")]
    text = open(tmp_path / "log" / "td.txt").read()
    assert "Validation" not in text and "valid_freq=0" in text
