"""Child of test_gpu_convbf_instances.test_convbf_switch_in_a_fresh_process.

    python tests/_convbf_switch_child.py SWITCH OUT.json

Started with the environment of SWITCH_CASES[SWITCH] (tests/
_convbf_instance_cases.py); the library reads MDE_CONVBF_RES / _RESMODE / _NW8
once per process.  Runs every forward and data-gradient case of the lists, and
the cases of the ids that exist only under the switch, against float64 under
guarded_abi() (tests/_convbf_instance_check.py), and writes one record a case:
the instance id the query reports in THIS process, the id the case is listed
for (switch-only cases), and whether it passed.  A failed comparison is
recorded and the run goes on; anything else (a HIP error) ends it at once.
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main(argv):
    switch, out = argv[0], argv[1]
    from tests import _convbf_instance_cases as cc
    from tests import _convbf_instance_check as ck
    env, fwd, dgrad = cc.SWITCH_CASES[switch]
    for k, v in env.items():
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    import monocular_depth_estimation_amd  # noqa: F401
    report = []
    todo = [(0, c, False) for c in cc.FWD_CASES] + [(1, c, False) for c in cc.DGRAD_CASES] + \
           [(0, c, True) for c in fwd] + [(1, c, True) for c in dgrad]
    for pass_, (shape, row, props), only in todo:
        got, info = ck.query(shape, pass_)
        rec = {"pass": pass_, "shape": list(shape), "id": got, "want": row if only else None,
               "kernel": info.get("kernel"), "tw": info.get("tw"), "nw": info.get("nw"), "ok": False}
        try:
            assert got >= 0, "refused under the switch"
            if only:
                ck.assert_listed(shape, pass_, row, props)
            rec["ratio"] = ck.run_forward(shape) if pass_ == 0 else ck.run_dgrad(shape)
            rec["ok"] = True
        except AssertionError as e:
            rec["error"] = str(e)[:500]
        print(switch, rec, flush=True)
        report.append(rec)
    with open(out, "w") as f:
        json.dump(report, f)
    print(f"DONE {switch}: {sum(r['ok'] for r in report)} of {len(report)} passed")


if __name__ == "__main__":
    main(sys.argv[1:])
