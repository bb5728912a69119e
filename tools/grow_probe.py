"""jsp_place_grow beside jsp_place_preempt on configs 2 and 5: C-timed calls and the launches' device time."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from jobset_amd import synth
from jobset_amd.engine import Engine
from jobset_amd.snapshot import job_runs

e = Engine(0)
out = []
for cfg in (2, 5):
    p = synth.CONFIGS[cfg]()
    e.load(p)
    rc, rl = job_runs(p.job_class)
    for name, t in (("grow", synth.grow_templates(p, 3)), ("fixed", synth.grow_templates(p, 3, fixed=1.0))):
        for _ in range(2):
            tot, med, p99 = e.place_grow_loop(rc, rl, t, iters=300)
        st = e.place_grow_runs(rc, rl, t)[5]
        dev = [e.grow_table(t, form, iters=200)[4] for form in (0, 1, 2)]
        out.append(dict(cfg=cfg, templates=name, grow_med_us=med, grow_p99_us=p99, placed=int(st.placed), grown=int(st.grown),
                        nodes=int(st.nodes), table_dev_us_form0=dev[0], table_dev_us_form1=dev[1], table_dev_us_form2=dev[2]))
    none = np.zeros(0, dtype=np.int32)
    for _ in range(2):
        tot, med, p99 = e.place_preempt_loop(rc, rl, 0, none, none.astype(np.uint32), iters=300)
    out.append(dict(cfg=cfg, preempt_med_us=med, preempt_p99_us=p99))
e.close()
for r in out:  # one JSON line per leg (profiles/grow/grow_probe.jsonl keeps a run's)
    print(json.dumps(r))
