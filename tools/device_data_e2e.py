"""End-to-end training throughput of train_no_amp with the DataLoader path (--device_data off) against device-prepared batches
(--device_data cache): --synthetic N subjects, batch 2, 128^3 crops, plan step mode.  Each mode runs in a child process; Trainer.step
is timed there from the end of the warm-up iterations to a device synchronise after the last one, and volumes/s is printed per mode.
With --device_data cache the subjects are generated at 240 x 240 x 155 and cropped on the device; the DataLoader path generates its
128^3 patches (with CPU edge codes) in its workers, as it does today.  usage: python tools/device_data_e2e.py [--iters N] [--warmup W]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd")


def child(mode, iters, warmup, subjects, workers):
    sys.path.insert(0, PKG)
    import torch
    import train_no_amp as T
    from cwf import trainer
    stamps = []
    step = trainer.Trainer.step

    def timed(self, *a, **k):
        out = step(self, *a, **k)
        if len(stamps) in (warmup - 1, warmup + iters - 1):
            torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        return out

    trainer.Trainer.step = timed
    with tempfile.TemporaryDirectory() as d:
        T.main(["--synthetic", str(subjects), "--device_data", mode, "--batch_size", "2", "--step_mode", "plan",
                "--num_workers", str(workers), "--max_iters", str(warmup + iters), "--end_epoch", "1000", "--save_freq", "100000",
                "--log_every", "1000000", "--project_root", d, "--aug_flip", "1" if mode != "off" else "0"])
    dt = stamps[warmup + iters - 1] - stamps[warmup - 1]
    print(json.dumps({"device_data": mode, "iters": iters, "volumes_per_s": round(2 * iters / dt, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--subjects", type=int, default=8)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.iters, args.warmup, args.subjects, args.workers)
    for mode in ("cache", "off"):
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", mode, "--iters", str(args.iters), "--warmup",
                               str(args.warmup), "--subjects", str(args.subjects), "--workers", str(args.workers)])


if __name__ == "__main__":
    main()
