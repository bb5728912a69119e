#!/usr/bin/env python3
"""Phase timelines from the diagnostic stamp build (make diag:
tools/bin/diag/libjsplace.so, jsp_stamps.h): the kernels store 100 MHz
s_memrealtime stamps (or s_memtime shader cycles) into 4096 rows of 8 slots --
a row per workgroup or wave, or a fixed row of one kernel -- and each
subcommand launches placements through the device path and prints medians
over launches.

  stamps.py phases [cfg=2] [reps=50] [b2b=1]   single-launch compaction, per workgroup
  stamps.py assign [cfg=4] [reps=20]           assign_kernel, three-launch shape
  stamps.py level  [reps=20]                   assign_level_kernel on cfg4
  stamps.py walk   [cfg=5] [fused=0] [reps=20] the assignment walk and the tally tiles
  stamps.py words  [cfg=5] [fused=1] [reps=20] per-word cost of the register walker
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("JSP_LIB_PATH", os.path.join(ROOT, "tools", "bin", "diag", "libjsplace.so"))

ROWS, SLOTS = 4096, 8


def load_lib():
    """The stamp build, with its two exports bound."""
    from jobset_amd import native
    lib = native.lib()
    lib.jsp_debug_stamps.argtypes = [ctypes.c_void_p, ctypes.c_uint]
    lib.jsp_debug_clear.argtypes = []
    return lib


def samples(cfg, reps, fused=None, launches=1):
    """Loads config `cfg` and yields its run count, then `reps` times the
    [4096, 8] stamp table (uint64, one buffer reused: copy what is kept) of
    `launches` back-to-back device-path placements after a clear; the stamps
    keep the last launch's times."""
    import torch
    from jobset_amd import synth
    from jobset_amd.engine import Engine
    from jobset_amd.snapshot import job_runs
    lib = load_lib()
    p = synth.CONFIGS[cfg]()
    eng = Engine(0)
    eng.load(p)
    if fused is not None:
        eng.set_fused(bool(fused))
    rc, rl = job_runs(p.job_class)
    rct = torch.from_numpy(rc.astype(np.int32)).cuda()
    rlt = torch.from_numpy(rl.astype(np.int32)).cuda()
    out = torch.empty(p.n_jobs, dtype=torch.int32, device="cuda")
    buf = np.zeros(ROWS * SLOTS, dtype=np.uint64)
    yield rc.shape[0]
    for _ in range(reps):
        lib.jsp_debug_clear()
        torch.cuda.synchronize()
        for _ in range(launches):
            eng.place_device(rct.data_ptr(), rlt.data_ptr(), rc.shape[0], p.n_jobs, out.data_ptr(), 0)
        torch.cuda.synchronize()
        lib.jsp_debug_stamps(buf.ctypes.data, buf.shape[0])
        yield buf.reshape(ROWS, SLOTS)


def ints(argv, defaults):
    """Positional integer arguments, the missing ones from `defaults`."""
    return [int(x) for x in argv[:len(defaults)]] + list(defaults[len(argv):])


def phases(argv):
    """Single-launch compaction kernel, per workgroup: 0 entry, 1 first barrier
    (row loads + LDS staging), 2 tally done, 3 feasible-count scan, 4 look-back
    done, 5 end; inside the tally 6 row pass done, 7 leaf pass done. Each
    phase's start relative to the launch's first stamp (ns). b2b > 1: that many
    back-to-back launches per sample (GPU busy)."""
    cfg, reps, b2b = ints(argv, (2, 50, 1))
    it = samples(cfg, reps, launches=b2b)
    next(it)
    rows = []
    for st in it:
        st = st[st[:, 0] != 0].astype(np.int64)
        rows.append((st - st[:, 0].min()) * 10)  # ns
    arr = np.stack(rows[5:])  # [reps, blocks, 8]
    med = np.median(arr, axis=0)
    print(f"cfg{cfg} ({b2b} back-to-back launches per sample): {med.shape[0]} workgroups; phase start (ns, median over {arr.shape[0]} launches)")
    cols = [0, 1, 6, 7, 2, 3, 4, 5]
    print("phase:          entry  barrier1  rowpass  leafpass  tallied  scanned  lookback  end")
    for b in range(min(med.shape[0], 24)):
        print(f"  wg {b:4d}: " + "  ".join(f"{med[b][c]:8.0f}" for c in cols))
    print("  max     : " + "  ".join(f"{med.max(axis=0)[c]:8.0f}" for c in cols))
    for q in (10, 50, 90):
        print(f"  p{q:<2d} wgs : " + "  ".join(f"{np.percentile(med[:, c], q):8.0f}" for c in cols))
    late = np.nonzero(med[:, 0] > 2000)[0]
    print(f"  {late.size} workgroups enter > 2 us after the first: {late[:40].tolist()}")
    if late.size:
        print(f"  their entry (ns): {med[late[:40], 0].astype(int).tolist()}")
    # per-workgroup phase durations (tally launch: entry -> barrier1 -> rowpass -> leafpass -> end)
    d = lambda a, b: np.median(med[:, b] - med[:, a])
    print(f"  median wg durations (ns): to-barrier1 {d(0, 1):.0f}  rowpass {d(1, 6):.0f}  "
          f"leafpass {d(6, 7):.0f}  write-out {d(7, 5):.0f}  total {d(0, 5):.0f}")


def assign(argv):
    """assign_kernel in the three-launch shape: stamps at entry, after staging,
    after each run (up to 5), end -- ns relative to entry."""
    cfg, reps = ints(argv, (4, 20))
    it = samples(cfg, reps, fused=False, launches=3)
    n_runs = next(it)
    rows = []
    for st in it:
        k = st[4000:4009].astype(np.int64)
        rows.append((k - k[0, 0]) * 10)
    med = np.median(np.stack(rows[3:]), axis=0)
    print(f"cfg{cfg} assign_kernel ({n_runs} runs): [entry, staged, .., end]; then per long run of class c<8: "
          f"start, scanned, window published, walked, copied out (last step), end (ns)")
    print("  kernel: " + "  ".join(f"{x:8.0f}" for x in med[0]))
    for t in range(8):
        if st[4001 + t, 0] != 0:  # the last launch's table
            print(f"  class {t}: " + "  ".join(f"{x:8.0f}" for x in med[1 + t][:6]))


def level(argv):
    """assign_level_kernel on cfg4: entry, staged, after runs 1..5, end -- ns
    relative to entry."""
    (reps,) = ints(argv, (20,))
    it = samples(4, reps)
    next(it)
    rows = []
    for b in it:
        st = b[4050].astype(np.int64)
        sub = b[4051].astype(np.int64)
        rows.append(np.concatenate([(st - st[0]) * 10, (sub - st[0]) * 10]))
    med = np.median(np.stack(rows[3:]), axis=0)
    print("assign_level_kernel cfg4 (ns from entry): staged {:.0f} | runs {} | end {:.0f}".format(
        med[1], " ".join(f"{x:.0f}" for x in med[2:6]), med[7]), flush=True)
    print("  per run: scan done {} | records issued {}".format(
        " ".join(f"{x:.0f}" for x in med[8:12]), " ".join(f"{x:.0f}" for x in med[12:16])), flush=True)


def walk(argv):
    """The assignment walk: kernel entry/staged/end (row 4000) and, per block of
    64 runs of the register-resident walker, stamps at runs 0, 16, 32, 48 and
    the block end (rows 4010+). ns relative to the kernel's first stamp."""
    cfg, fused, reps = ints(argv, (5, 0, 20))
    it = samples(cfg, reps, fused=fused)
    n_runs = next(it)
    rows, clk = [], []
    for b in it:
        st = b.astype(np.int64)
        rt = st[:4090]  # real-time stamps (row 4090 mixes in shader-clock values)
        nz = rt[rt != 0]
        t0 = nz.min() if nz.size else 0
        sel = np.concatenate([st[4000:4050], st[0:64]])  # walk rows, then tally tiles 0..63
        rows.append(np.where(sel != 0, (sel - t0) * 10, -1))
        r = st[4090]
        if r[0] and r[2]:
            clk.append((r[2] - r[0]) / ((r[3] - r[1]) * 10.0))  # shader cycles per ns = GHz
    med = np.median(np.stack(rows[3:]), axis=0)
    print(f"cfg{cfg} fused={fused} runs={n_runs}: ns from the launch's first stamp; "
          f"effective shader clock over the walk {np.median(clk) if clk else float('nan'):.2f} GHz")
    for r in range(50):
        if (med[r] >= 0).any():
            print(f"  row {4000 + r}: " + "  ".join(f"{x:8.0f}" for x in med[r]))
    print("  tally tiles (0 entry, 1 staged, 6 row pass, 7 leaf pass, 5 published):")
    for r in range(50, 114):
        if (med[r] >= 0).any():
            print(f"  tile {r - 50:4d}: " + "  ".join(f"{med[r][i]:8.0f}" for i in (0, 1, 6, 7, 5)))


def words(argv):
    """Per-word cost of the register walker's first four batches -- shader
    cycles from word start to the end of the job chain and to the end of the
    word, jobs visited and domains taken. Rows 4020 + 4*batch + word
    (s_memtime cycles)."""
    cfg, fused, reps = ints(argv, (5, 1, 20))
    it = samples(cfg, reps, fused=fused)
    next(it)
    rows = [b[4020:4036].astype(np.int64) for b in it]
    a = np.stack(rows[3:])
    print(f"cfg{cfg} fused={fused}: per word of batches 1-4 (last tile): cycles chain / word, visits, taken")
    for r in range(16):
        x = a[:, r]
        if (x[:, 0] == 0).all():
            continue
        chain = np.median(x[:, 1] - x[:, 0])
        word = np.median(x[:, 2] - x[:, 0])
        print(f"  batch {r // 4 + 1} word {r % 4}: chain {chain:7.0f}  word {word:7.0f}  visits {int(np.median(x[:, 3])):3d}"
              f"  taken {int(np.median(x[:, 4])):3d}  cycles/visit {chain / max(1, np.median(x[:, 3])):6.1f}")


COMMANDS = {"phases": phases, "assign": assign, "level": level, "walk": walk, "words": words}

if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in COMMANDS:
        sys.exit(__doc__)
    COMMANDS[sys.argv[1]](sys.argv[2:])
