#!/usr/bin/env python3
"""Prints what RECORDED of tests/test_gpu_filter_call_plans.py holds, from the library in use (on an MI355X).  To re-record
after a deliberate change of the schedule, run it with the PARENT commit's library:
    RAGRAPH_HIP_SO=build_ab/lib_parent.so python tools/record_filter_call_plans.py"""
import os
import pprint
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_filter_call_plans as T  # noqa: E402

dev = torch.device("cuda", 0)
rec = {name: T.single_call_plan(dev, name, False) for name in sorted(T.SHAPES)}
rec.update({name + "+prior": T.single_call_plan(dev, name, True) for name in T.PRIOR_SHAPES})
rec["two_shards"] = T.sharded_call_plans(dev, *T.TWO_SHARDS, False)
rec["two_shards+prior"] = T.sharded_call_plans(dev, *T.TWO_SHARDS, True)
rec["three_shards"] = T.sharded_call_plans(dev, *T.THREE_SHARDS, False)
print("RECORDED = " + pprint.pformat(rec, width=120, sort_dicts=False))
