"""Time the class location tables of the foreground-oversampled crops (csrc/locations.hip) and count what the oversampling does, in one
process, every section under a time limit of its own (SIGALRM ends the process):
  * kernel: cwf_class_locations on one synthetic 240 x 240 x 155 subject, R = 3 (classes 1, 2, 3), K = 4096, hip events, medians of 5
    windows of 20 calls after a warm-up, against (a) the floor of TWO reads of the label at 6.3 TB/s, (b) the same table built with
    torch ops on the device in the same run (nonzero per region, then an index by the rank list; its result is compared) and (c) the
    numpy statement (utils.data.class_locations on the host, one thread, host clock, median of 5 calls);
  * dataset: the table building of DeviceBraTS(cache=True) for 8 such subjects (one call per subject into one tensor pair, one copy to
    the host), host clock around a device synchronise, median of 5;
  * shares: over 1000 draws (125 epochs of the 8 subjects), the share of 128^3 crops that hold each class with oversample 0 and 0.33.
    Counted on the host from draw_params' origins: it needs no GPU (--device cpu builds the tables with the numpy statement).
usage: python tools/foreground_micro.py [--what kernel,dataset,shares] [--device cuda:0] [--limit SECONDS]"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "decouple-and-couple_learning_in_multi-modal_brain_tumor_segmentation_amd"))

from utils import data  # noqa: E402
from utils import synthetic as syn  # noqa: E402

FULL, CROP = (240, 240, 155), (128, 128, 128)
HBM_BPS = 6.3e12
WINDOWS, CALLS = 5, 20
MASKS, K = data.FOREGROUND_CLASSES, 4096
SUBJECTS = 8


def windows_us(fn, warmup=3):
    """median and spread over WINDOWS windows of CALLS calls each, microseconds per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / CALLS * 1e3)
    return {"median_us": round(statistics.median(per), 2), "min_us": round(min(per), 2), "max_us": round(max(per), 2)}


def limited(seconds):
    def on_alarm(signum, frame):
        print(json.dumps({"error": "section ran past its %d s limit" % seconds}), flush=True)
        os._exit(124)
    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(seconds)


def labels(n):
    return [syn.synthetic_label(i, FULL).to(torch.uint8).contiguous() for i in range(n)]


def torch_statement(lab):
    """the same table with torch ops on the device: nonzero per region (a host synchronisation each), then an index by the rank list"""
    flat = lab.reshape(-1)
    flat = torch.where(flat == 4, torch.full_like(flat, 3), flat)
    counts = torch.zeros(len(MASKS), dtype=torch.int64, device=lab.device)
    table = torch.full((len(MASKS), K), -1, dtype=torch.int32, device=lab.device)
    for r, mk in enumerate(MASKS):
        member = torch.zeros_like(flat, dtype=torch.bool)
        for c in range(4):
            if (mk >> c) & 1:
                member |= flat == c
        where = member.nonzero().reshape(-1)
        n = int(where.numel())
        m = min(n, K)
        counts[r] = n
        if m:
            table[r, :m] = where[(torch.arange(m, dtype=torch.int64, device=lab.device) * n) // m].to(torch.int32)
    return counts, table


def kernel_section(out, dev):
    from cwf import kernels
    B = kernels.backend()
    host = labels(1)[0]
    lab = host.to(dev)
    V = lab.numel()
    counts = torch.empty(len(MASKS), dtype=torch.int64, device=dev)
    table = torch.empty((len(MASKS), K), dtype=torch.int32, device=dev)
    B.class_locations(lab, MASKS, K, out=(counts, table))
    tc, tt = torch_statement(lab)
    hc, ht = data.class_locations(host, MASKS, K)
    out["counts"] = counts.tolist()
    out["equal_to_torch"] = bool(torch.equal(counts, tc) and torch.equal(table, tt))
    out["equal_to_numpy"] = bool(torch.equal(counts.cpu(), hc) and torch.equal(table.cpu(), ht))
    floor_us = 2 * V / HBM_BPS * 1e6
    k = windows_us(lambda: B.class_locations(lab, MASKS, K, out=(counts, table)))
    k.update(two_reads_floor_us=round(floor_us, 2), times_floor=round(k["median_us"] / floor_us, 1))
    t = windows_us(lambda: torch_statement(lab))
    k["times_torch"] = round(k["median_us"] / t["median_us"], 4)
    per = []
    for _ in range(5):
        t0 = time.perf_counter()
        data.class_locations(host, MASKS, K)
        per.append((time.perf_counter() - t0) * 1e6)
    out["cwf_class_locations"], out["torch_on_device"] = k, t
    out["numpy_on_host"] = {"median_us": round(statistics.median(per), 1), "min_us": round(min(per), 1), "max_us": round(max(per), 1)}


def dataset_section(out, dev):
    image = torch.zeros((4,) + FULL)                                   # the images play no part in the tables: one block of zeros for all
    ds = data.DeviceBraTS([(image, lab) for lab in labels(SUBJECTS)], dev, CROP, cache=True, oversample=0.33, foreground_samples=K)
    per = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds._locate_all()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e3)
    out["tables_of_%d_subjects" % SUBJECTS] = {"median_ms": round(statistics.median(per), 3), "min_ms": round(min(per), 3),
                                               "max_ms": round(max(per), 3)}
    out["counts"] = [c.tolist() for c, _ in ds.foreground]


def shares_section(out, dev):
    labs = labels(SUBJECTS)
    fg = [tuple(t.cpu().numpy() for t in data.class_locations(lab.to(dev), MASKS, K)) for lab in labs]
    arrs = [lab.numpy() for lab in labs]
    draws = 1000
    for p in (0.0, 0.33):
        held, moved = np.zeros(4, dtype=np.int64), 0
        for d in range(draws):
            epoch, i = divmod(d, SUBJECTS)
            o = data.draw_params(1000, epoch, i, FULL, CROP, oversample=p, foreground=fg[i] if p > 0.0 else None).origin
            moved += o != data.draw_params(1000, epoch, i, FULL, CROP).origin
            crop = arrs[i][o[0]:o[0] + CROP[0], o[1]:o[1] + CROP[1], o[2]:o[2] + CROP[2]]
            held += np.bincount(crop.reshape(-1), minlength=5)[:4] > 0
        out["oversample_%g" % p] = {"draws": draws, "origins_moved": int(moved),
                                    "share_with_class": {str(c): round(float(held[c]) / draws, 4) for c in (1, 2, 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernel,dataset,shares")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--limit", type=int, default=240, help="seconds each section may take")
    a = ap.parse_args()
    sections = {"kernel": kernel_section, "dataset": dataset_section, "shares": shares_section}
    for what in a.what.split(","):
        if what not in sections:
            raise SystemExit("unknown section %r" % what)
        if what != "shares" and not a.device.startswith("cuda"):
            raise SystemExit("section %r times the device: it needs a GPU" % what)
        out = {}
        limited(a.limit)
        sections[what](out, a.device)
        signal.alarm(0)
        print(json.dumps({what: out}), flush=True)


if __name__ == "__main__":
    main()
