"""Evaluate a checkpoint on whole subjects -- what the reference's test_overlap.py / test_all_pth.py report, on the device:

    python evaluate.py --resume checkpoint/.../model_best.pth --root dataset --valid_dir Valid --valid_file valid.txt --out eval
    python -m torch.distributed.run --nproc-per-node 8 evaluate.py --resume ... --out eval        (cases sharded over the ranks)

The model is built, the checkpoint loaded (load_checkpoint; --use_ema takes the EMA weights it carries) and a cwf.validation.Validator
run over the subjects: sliding windows of --crop_H/W/D, the --overlap / --crop_nonzero / --tta / --postprocess / --hd95 settings of
train_no_amp.py's --valid_* flags.  Rank 0 writes DIR/cases.csv (one row per case: name, Dice of WT / TC / ET, IoU of classes 1..3,
the counts they are ratios of, the voxel count and the optional metrics) and DIR/summary.json (the aggregates of
cwf.validation.ValidationResult and the settings).  --save_seg writes each label map as DIR/<name>.npy, uint8 with class 3 written as 4,
the BraTS value.  --lesionwise and --nsd T1,T2 add predict_overlap.lesionwise_metrics and surface_regions per case; they read their
results back case by case.  NIfTI output is not provided."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

LESION_COLUMNS = tuple("lesion_%s_%s" % (m, r) for m in ("dice", "hd95") for r in ("wt", "tc", "et"))


def _bool(v):
    return str(v).strip().lower() not in ("", "0", "false", "no", "off")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--resume", required=True, type=str, help="the checkpoint to evaluate")
    p.add_argument("--use_ema", default=False, type=_bool, help="evaluate the checkpoint's EMA weights ('ema_state_dict')")
    p.add_argument("--root", default="dataset", type=str)
    p.add_argument("--valid_dir", default="Valid", type=str)
    p.add_argument("--valid_file", default="valid.txt", type=str)
    p.add_argument("--synthetic", default=0, type=int, help="evaluate on M generated subjects of (input_H, input_W, output_D) voxels")
    p.add_argument("--synthetic_first", default=0, type=int, help="(--synthetic) index of the first generated subject")
    p.add_argument("--seed", default=1000, type=int)
    p.add_argument("--dataset", default="brats", type=str)
    p.add_argument("--input_H", default=240, type=int)
    p.add_argument("--input_W", default=240, type=int)
    p.add_argument("--output_D", default=155, type=int)
    p.add_argument("--crop_H", default=128, type=int)
    p.add_argument("--crop_W", default=128, type=int)
    p.add_argument("--crop_D", default=128, type=int)
    p.add_argument("--precision", default="bf16x3", choices=("fp32", "bf16x3", "bf16"))
    p.add_argument("--normalize", default=False, type=_bool, help="z-score each subject's channels over its brain mask, as in training")
    p.add_argument("--overlap", default=0.5, type=float)
    p.add_argument("--crop_nonzero", default=False, type=_bool)
    p.add_argument("--tta", default=False, type=_bool)
    p.add_argument("--postprocess", default="none", choices=("none", "reference"))
    p.add_argument("--hd95", default=False, type=_bool)
    p.add_argument("--cache", default=False, type=_bool, help="hold every subject in device memory before the run (default: load each in turn)")
    p.add_argument("--lesionwise", default=False, type=_bool, help="add lesion-wise Dice and HD95 per case (BraTS 2023)")
    p.add_argument("--nsd", default=None, type=str, help="T1,T2,...: add the normalised surface Dice at these tolerances (at most 4) per case")
    p.add_argument("--out", required=True, type=str, help="directory of cases.csv, summary.json and the label maps")
    p.add_argument("--save_seg", default=False, type=_bool)
    p.add_argument("--local_rank", default=int(os.environ.get("LOCAL_RANK", 0)), type=int)
    p.add_argument("--backend", default=None, type=str)
    return p


def check_args(args):
    if not os.path.isfile(args.resume):
        raise SystemExit("--resume %s: no such checkpoint" % args.resume)
    if not 0.0 <= args.overlap < 1.0:
        raise SystemExit("--overlap takes an overlap in [0, 1)")
    if args.synthetic < 0 or args.synthetic_first < 0:
        raise SystemExit("--synthetic / --synthetic_first take numbers >= 0")
    tol = ()
    if args.nsd is not None:
        try:
            tol = tuple(float(t) for t in args.nsd.split(",") if t.strip())
        except ValueError:
            raise SystemExit("--nsd takes comma-separated tolerances, got %r" % args.nsd)
        if not 1 <= len(tol) <= 4 or any(not t >= 0.0 for t in tol):
            raise SystemExit("--nsd takes one to four tolerances >= 0")
    from predict_overlap import check_roi
    try:
        check_roi((args.crop_H, args.crop_W, args.crop_D))
    except ValueError as e:
        raise SystemExit("--crop_H / --crop_W / --crop_D: %s" % e)
    return tol


def subjects_of(args):
    if args.synthetic > 0:
        from utils import synthetic as syn
        full = (args.input_H, args.input_W, args.output_D)
        vols = [syn.synthetic_volume(args.synthetic_first + j, full, args.seed) for j in range(args.synthetic)]
        return [(x, t.to(torch.uint8)) for x, t in vols]
    from utils.data import _npz_paths
    root = os.path.join(args.root, args.valid_dir)
    lst = os.path.join(root, args.valid_file)
    try:
        return _npz_paths(root, lst if os.path.isfile(lst) else None)
    except FileNotFoundError as e:
        raise SystemExit("no subjects to evaluate (%s): give --root / --valid_dir / --valid_file, or --synthetic M" % e)


def main(argv=None):
    args = build_parser().parse_args(argv)
    tol = check_args(args)
    subjects = subjects_of(args)
    if not torch.cuda.is_available():
        raise SystemExit("evaluate.py runs on the device kernels only: no GPU is available")
    from cwf import kernels
    from cwf.trainer import load_checkpoint
    from cwf.validation import Validator, write_cases_csv, write_json
    from models.clswiseformer.cls_wise_former import get_cls_wise_former
    import predict_overlap as po

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(args.backend or "nccl")
    device = torch.device("cuda", args.local_rank)
    torch.cuda.set_device(device)
    kernels.set_precision(args.precision)
    model = get_cls_wise_former(dataset=args.dataset, _conv_repr=True, _pe_type="fixed", gpu=args.local_rank).to(device)
    load_checkpoint(args.resume, model, use_ema=args.use_ema)
    model.eval()

    window = {"roi_size": (args.crop_H, args.crop_W, args.crop_D), "overlap": args.overlap}
    if args.crop_nonzero:
        window["crop_nonzero"] = True
    validator = Validator(subjects, device, window=window, use_tta=args.tta,
                          postprocess=po.REFERENCE_POSTPROCESS if args.postprocess == "reference" else None, normalize=args.normalize,
                          cache=args.cache, with_hd95=args.hd95, rank=rank, world=world)
    os.makedirs(args.out, exist_ok=True)
    extra_names = (LESION_COLUMNS if args.lesionwise else ()) + tuple("nsd_%s_%g" % (r, t) for r in ("wt", "tc", "et") for t in tol)
    extras = torch.zeros((len(validator), len(extra_names)), dtype=torch.float64, device=device)

    def on_case(i, seg, target, prob):
        if args.save_seg:
            lab = seg[0].to(torch.uint8)
            np.save(os.path.join(args.out, validator.names[i] + ".npy"), torch.where(lab == 3, torch.full_like(lab, 4), lab).cpu().numpy())
        col = 0
        if args.lesionwise:
            lw = po.lesionwise_metrics(seg, target.long())
            extras[i, 0:3], extras[i, 3:6] = lw["dice"][0].to(torch.float64), lw["hd95"][0].to(torch.float64)
            col = 6
        if tol:
            extras[i, col:] = po.surface_regions(seg, target.long(), tol)["nsd"][0].reshape(-1)

    result = validator.run(model, on_case=on_case if (args.save_seg or extra_names) else None)
    if world > 1 and extra_names:
        dist.all_reduce(extras, op=dist.ReduceOp.SUM)          # rows of other ranks are zero, as in the Validator's table
    if rank == 0:
        rows = result.to_rows()
        if extra_names:
            host = extras.cpu().numpy()
            for row, vals in zip(rows, host):
                row.update((n, float(v)) for n, v in zip(extra_names, vals))
        write_cases_csv(os.path.join(args.out, "cases.csv"), rows)
        summary = result.to_json()
        if extra_names and len(rows):
            summary["extra_mean"] = {n: float(np.nanmean(host[:, k])) if not np.all(np.isnan(host[:, k])) else float("nan")
                                     for k, n in enumerate(extra_names)}
        summary["settings"] = {k: v for k, v in sorted(vars(args).items())}
        summary["world"] = world
        write_json(os.path.join(args.out, "summary.json"), summary)
        print("evaluated %d cases: dice WT %.5f TC %.5f ET %.5f, score %.5f -> %s" % (
            len(result), *result.dice_stats["mean"], result.score, args.out))
    if world > 1 and dist.is_initialized():
        dist.barrier()
    return 0


if __name__ == "__main__":
    sys.exit(main())
