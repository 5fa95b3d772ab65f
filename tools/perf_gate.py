#!/usr/bin/env python3
"""GPU perf gate: ~70 chains against committed per-chain ceilings (tools/perf_ceilings.json, microseconds per launch / update / batch).

Round 2 shipped a 1.4-7x slowdown of one kernel family with every bit-exactness test green.  The static half of
the answer is tests/test_kernel_resources.py (CPU, metadata of the built kernels); this is the measured half: the reference's
own test chains at the reference's sizes (tools/bench_reference_tests.py), BASELINE's cfg #3 / #4 and the decode-side batches
(tools/bench_more.py), whole-frame resizes, the headline on the queue AND as one launch per step, cfg #3 on the queue and the
stream-ordered tick regime are timed and compared with the ceilings.

Round 3's ceilings were max(1.25 x, + 8 us) and never under 13 us: a 4.4 us launch at 13.0, every 3-6 us chain at 13-15 -- the gate caught
round 2's 5 x and nothing subtler.  The reason was the CLOCK, not the kernels: 60 eager calls timed once from Python.
Every row is now device time from a replayed HIP graph, median of 3 (bench_reference_tests.timed), and a ceiling is
    max(1.25 x median, median + 1.5 us)                       (stream-ordered rows, paced by the runtime's stream scheduling: 1.6 x)
-- a 1.5 x slip of any chain of 6 us or more fails, a 3.4 us chain fails at 4.9 us.  tests/test_gpu_perf_gate.py holds the gate to that:
a deliberately bad knob (K1 forced to 4 rows per wave, the four-pixel up-scaling kernel switched off) must fail it.

  python tools/perf_gate.py                  # run on the GPU box, print a JSON verdict, exit 0 / 1
  python tools/perf_gate.py --quick          # the subset the GPU test runs (headline launch, K1 batches, up-scaling): seconds
  python tools/perf_gate.py --write          # measure 3 times and REWRITE the ceilings from the per-row medians
  python tools/perf_gate.py --rows f.jsonl   # gate rows measured elsewhere (JSON lines with test|config and us*)
bench.py's extras call check() on the rows they measured anyway, so the driver's BENCH line carries the verdict too."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tools", "perf_ceilings.json")
SLACK = 1.25
ABS_SLACK_US = 1.5
STREAM_SLACK = 1.6  # rows whose pace is the runtime's stream scheduling (stream-ordered submission): wider


def eager_row(name):
    """rows that cannot be replayed from a graph (a default CircularTensor handle's update, host descriptor tables): timed as eager calls,
    i.e. paced by the host -- the mirrored ring's 4K -> 1080p push read 14.5 ... 19.7 us between runs of one tree"""
    return (name.startswith("cfg4") and "CAPTURABLE" not in name) or "eager" in name or "host descriptors" in name


def ceiling(name, us):
    if name.startswith("stream-ordered"):
        return round(max(us * STREAM_SLACK, us + ABS_SLACK_US), 2)
    if eager_row(name):
        return round(max(us * SLACK, us + 6.0), 2)
    return round(max(us * SLACK, us + ABS_SLACK_US), 2)


def key_us(row):
    """(name, microseconds) of a row from bench_reference_tests / bench_more / bench.py"""
    name = row.get("test") or row.get("config") or row.get("name")
    for k in ("us", "us_per_update", "us_per_launch", "us_per_step"):
        if k in row:
            return name, float(row[k])
    return name, None


def check(rows, table=None):
    table = table if table is not None else json.load(open(TABLE))
    over, new, ok = [], [], 0
    for r in rows:
        name, us = key_us(r)
        if name is None or us is None:
            continue
        ceil = table.get(name)
        if ceil is None:
            new.append(name)
        elif us > ceil:
            over.append({"chain": name, "us": us, "ceiling_us": ceil})
        else:
            ok += 1
    return {"checked": ok + len(over), "over": over, "new": new, "pass": not over}


def headline_rows():
    """the headline on bench.py's own clocks: the queue (one submit per step), one graph-replayed launch per step, the stream-ordered ticks"""
    import subprocess
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--no-cpu", "--no-extra", "--no-regimes"], capture_output=True, text=True)
    rows = []
    try:
        j = json.load(open(os.path.join(ROOT, "bench_extra.json")))
        rows.append({"name": "headline cfg2b 50 crops, one cvgs_queue_submit per step (bench.py clock)", "us_per_step": j["timing"]["step_us_median"]})
        rows.append({"name": "headline cfg2b 50 crops, one launch per step (bench.py clock)", "us_per_step": j["one_launch_per_step"]["us_per_step"]})
    except Exception as ex:
        sys.stderr.write("perf_gate: no headline rows (%r)\n%s\n" % (ex, p.stderr[-2000:]))
    return rows


def stream_rows():
    """in a fresh process (these rows are paced by the runtime's stream scheduling, which depends on the process's history)"""
    import subprocess
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_queue_regimes.py"), "--json", "--only-stream"], capture_output=True, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if not line:
        sys.stderr.write("perf_gate: no stream-ordered rows\n%s\n" % p.stderr[-1000:])
        return []
    r = json.loads(line[-1])["stream_ordered"]
    return [{"name": "stream-ordered: ticks of 16 frames behind one gate, 1 stream, wait deferred 2 ticks, producer on the stream", "us": r["ticks_of_16_on_1_stream_wait_deferred_2_ticks"]["us"]},
            {"name": "stream-ordered: ticks of 16 frames behind one gate, 2 streams, producer on the stream", "us": r["ticks_of_16_on_2_streams"]["us"]},
            {"name": "stream-ordered: lone stream, hybrid policy (direct launch), producer on the stream", "us": r["lone_stream_hybrid"]["us"]}] + [
            {"name": "stream-ordered: ticks of 16 frames as ONE cvgs_execute_many launch, %s, no queue, producer on the stream" % lab, "us": r[k]["us"]}
            for k, lab in (("ticks_of_16_one_launch_1_stream", "1 stream"), ("ticks_of_16_one_launch_2_streams", "2 streams")) if k in r]


def quick_rows():
    """the subset tests/test_gpu_perf_gate.py runs: K1 as one launch per step (bench.py's graph clock), the reference's 50-crop batch chains and
    the whole-frame up-scaling kernel -- what the CVGS_K1_RPW / CVGS_K1_X4 knobs move"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch
    import bench as B
    import bench_upscale
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    torch.cuda.set_stream(torch.cuda.Stream())
    wl = B.Workload(dev, 20, 50, 0, 1, False)
    ts = sorted(B.measure(wl, 256, 16, target_s=0.05, min_replays=10)["step_s"] for _ in range(3))
    rows = [{"name": "headline cfg2b 50 crops, one launch per step (bench.py clock)", "us_per_step": round(ts[1] * 1e6, 3)}]
    del wl
    torch.cuda.empty_cache()
    for src, dst in bench_upscale.CASES[:3]:
        r = bench_upscale.case(dev, 3, src, dst, 100)
        rows.append({"name": "resize packed " + r["case"], "us": r["us"]})
    return rows


def measure_all():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch
    import bench_more
    import bench_reference_tests
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    rows = bench_reference_tests.run_all(verbose=False)
    torch.cuda.empty_cache()
    torch.cuda.set_stream(torch.cuda.Stream())
    rows += bench_more.run_all(dev, iters=60)
    torch.cuda.empty_cache()
    import bench_upscale  # whole-frame resizes into packed u8 (K1's four-pixels-per-lane form and its down-scaling sibling)
    for src, dst in bench_upscale.CASES:
        r = bench_upscale.case(dev, 3, src, dst, 100)
        rows.append({"name": "resize packed " + r["case"], "us": r["us"]})
    torch.cuda.empty_cache()
    rows += stream_rows()
    rows += headline_rows()
    return rows


def main(argv):
    write = "--write" in argv
    quick = "--quick" in argv
    if "--rows" in argv:
        rows = [json.loads(l) for l in open(argv[argv.index("--rows") + 1]) if l.startswith("{")]
    elif write:  # three full passes, the per-row median
        passes = [measure_all() for _ in range(3)]
        by = {}
        for rows_ in passes:
            for r in rows_:
                name, us = key_us(r)
                if name and us:
                    by.setdefault(name, []).append(us)
        rows = [{"name": k, "us": sorted(v)[len(v) // 2]} for k, v in by.items()]
    else:
        rows = quick_rows() if quick else measure_all()
    if write:
        table = {}
        for r in rows:
            name, us = key_us(r)
            if name and us:
                table[name] = ceiling(name, us)
        with open(TABLE, "w") as f:
            json.dump(table, f, indent=0, sort_keys=True)
        with open(TABLE.replace(".json", "_measured.json"), "w") as f:
            json.dump({key_us(r)[0]: key_us(r)[1] for r in rows}, f, indent=0, sort_keys=True)
        print("wrote %d ceilings to %s" % (len(table), TABLE))
        return 0
    v = check(rows)
    v["rows"] = [dict(zip(("chain", "us"), key_us(r))) for r in rows]
    print(json.dumps(v))
    return 0 if v["pass"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
