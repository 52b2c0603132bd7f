#!/usr/bin/env python3
"""Where the last mmc_batch_run call of a rocprofv3 kernel trace spends its time.

    python scripts/call_timeline.py run_kernel_trace.csv [--moves N] [--full-rate MOVES_PER_S]

The call is the last run of kernels that ends with the commit of the last step (k_settle /
k_settle_rec) and begins after the previous call's commit.  Printed: every kernel of the call
(start and end in microseconds from the call's first kernel), then the split of the call's kernel
window into
  move kernels alone       k_move_eval_wave running, one launch at a time
  move kernels overlapped  two move launches resident together (a launch's tail and the next one's ramp)
  other kernels            k_propose, k_fetch_bytes, commits -- not under a move kernel
  idle                     nothing running on the device
With --moves and --full-rate (moves per second of a long call, where fixed costs vanish), the
window is also set against the time the call's moves take at that rate: the rest is what the
call's shape costs on the device (tails, ramps, gaps, auxiliary kernels).  Host time before the
first and after the last kernel is not in a kernel trace: see MMC_RUN_TRACE.
"""
import argparse
import csv


def short(name):
    return name.split("(")[0].replace("void ", "")


def load(path):
    with open(path) as f:
        rows = list(csv.DictReader(f))
    ks = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in rows]
    return sorted(ks)


def last_call(ks):
    settle = [i for i, k in enumerate(ks) if k[2].startswith("k_settle")]
    if not settle:
        raise SystemExit("no k_settle in the trace: no driver call")
    end = settle[-1]
    # the commits of one call are adjacent in launch order; the call starts after the previous call's
    i = end
    while i > 0 and ks[i - 1][2].startswith("k_settle"):
        i -= 1
    j = i - 1
    while j >= 0 and not ks[j][2].startswith("k_settle"):
        j -= 1
    first = j + 1
    # (kernels of other work -- totals, copies -- between two calls are not the call's)
    while first < i and ks[first][2].split("<")[0] not in ("k_fetch_bytes", "k_propose", "k_move_eval_wave"):
        first += 1
    return ks[first:end + 1]


def split(call):
    t0 = call[0][0]
    t1 = max(k[1] for k in call)
    ev = []
    for s, e, n in call:
        kind = "move" if n.startswith("k_move_eval_wave") else "other"
        ev += [(s, 1, kind), (e, -1, kind)]
    ev.sort(key=lambda x: (x[0], x[1]))
    cnt = {"move": 0, "other": 0}
    acc = {"move_alone": 0, "move_overlapped": 0, "other": 0, "idle": 0}
    last = t0
    for t, d, kind in ev:
        dt = t - last
        if dt > 0:
            if cnt["move"] >= 2:
                acc["move_overlapped"] += dt
            elif cnt["move"] == 1:
                acc["move_alone"] += dt
            elif cnt["other"] > 0:
                acc["other"] += dt
            else:
                acc["idle"] += dt
        cnt[kind] += d
        last = t
    return t0, t1, acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--moves", type=float, default=0)
    ap.add_argument("--full-rate", type=float, default=0)
    a = ap.parse_args()
    call = last_call(load(a.trace))
    t0, t1, acc = split(call)
    for s, e, n in call:
        print(f"  {n:20s} {(s - t0) / 1e3:9.1f} .. {(e - t0) / 1e3:9.1f} us  ({(e - s) / 1e3:8.1f})")
    win = (t1 - t0) / 1e3
    print(f"kernel window {win:.1f} us, move launches {sum(1 for k in call if k[2].startswith('k_move_eval_wave'))}")
    for k, v in acc.items():
        print(f"  {k:16s} {v / 1e3:9.1f} us  {100 * v / 1e3 / win:5.1f} %")
    if a.moves and a.full_rate:
        ideal = 1e6 * a.moves / a.full_rate
        print(f"  at {a.full_rate:.4g} moves/s the call's moves take {ideal:.1f} us: the shape costs "
              f"{win - ideal:.1f} us of the window")


if __name__ == "__main__":
    main()
