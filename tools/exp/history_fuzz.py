"""Call-history fuzz of ONE long-lived context over every entry family (tests/history_cases.py, the walk of tests/test_gpu_history.py at
any length): each step is a random action in a random form, a dense call on a random batch of 1 to 4 pairs, an excursion (a setting or a
cache changed, work under it, the baseline restored) or a refusal; asynchronous results are collected up to three steps later; every
result is compared bit for bit with its expectation from the CPU restatements.  What it hunts: a result that depends on what ran before
it.  python tools/exp/history_fuzz.py [steps] [seed] [arith: opencv | legacy]"""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
capi = importlib.import_module("uw-slam_amd.capi")
from oracle import oracle as O
import history_cases as HC

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
arith = sys.argv[3] if len(sys.argv) > 3 else ("opencv", "legacy")[seed % 2]
capi.DEFAULT_ARITH = O.DEFAULT_ARITH = HC.ARITH[arith]
O.build()
O.set_arith(HC.ARITH[arith])
t0 = time.time()
world = HC.make_world()
rig = HC.Rig(capi, world)
trail = []
failures = HC.random_walk(rig, arith, steps, seed, log=trail.append)
rig.close()
for f in failures[:40]:
    print(f)
print("history_fuzz seed %d (%s): %d steps, %d differ (%.1f s)" % (seed, arith, steps, len(failures), time.time() - t0))
sys.exit(1 if failures else 0)
