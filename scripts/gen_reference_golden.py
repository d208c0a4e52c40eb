#!/usr/bin/env python3
"""Record the reference-compatibility fixtures under tests/golden/reference/.

The compatibility tests compare this framework against DATA the reference
(uw-mad-dash/shockwave) ships or produces: its 120-job trace, its V100
throughput oracle, its committed simulation results, the batch-size
schedules its oracle functions return, and the bytes its protobuf
messages serialize to.  This script reads a reference checkout ONCE and
stores only that data (no reference code, no .proto text), so the tests
run from this repository alone.

  python scripts/gen_reference_golden.py --reference /path/to/shockwave

Files written (tests/golden/reference/):
  trace_120.trace        the reference's 120-job trace, verbatim
  tacc_throughputs.json  the isolated V100 rates of its throughput oracle
                         (the parity tests run v100 without packing, so
                         other worker types and pair rates are never read)
  tacc_32gpus.json       its shockwave solver settings, verbatim
  sim_results.json       makespan / avg JCT / rho list of its result pickles
  bs_patterns.json       outputs of its two batch-size oracle functions,
                         run-length encoded as [[batch size, epochs], ...]
  proto_fields.json      (name, number, repeated) of every message field,
                         and the enum numbering
  wire_messages.json     payload -> hex bytes as serialized by message
                         classes built from the reference's schema
"""

import argparse
import ast
import json
import os
import pickle
import shutil
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)

OUT = os.path.join(REPO, "tests", "golden", "reference")

TRACE_NAME = (
    "120_0.2_5_100_40_25_0,0.5,0.5_0.6,0.3,0.09,0.01_multigpu_dynamic"
)
SIM_POLICIES = ("max_min_fairness", "allox", "shockwave")

GNS_EPOCHS = (1, 5, 12, 31, 59, 100, 200, 400)
ACCORDION_EPOCHS = (1, 10, 31, 100, 270)
ACCORDION_COMBOS = (
    [("ResNet-18", b) for b in (16, 32, 64, 128, 256)]
    + [("ResNet-50", b) for b in (16, 32, 64)]
    + [("Transformer", b) for b in (16, 32, 64, 128)]
    + [("LM", b) for b in (5, 10, 20, 40, 80)]
    + [("Recommendation", b) for b in (512, 2048, 8192)]
)

# payloads the wire tests exchange with the reference's message classes
WIRE_PAYLOADS = {
    "DoneRequest": {
        "worker_id": 3, "job_id": [1, 2], "num_steps": [10, 20],
        "execution_time": [1.5, 2.5], "iterator_log": ["a", "b"],
    },
    "UpdateLeaseResponse": {
        "max_steps": 500, "max_duration": 120.5, "extra_time": 7.25,
        "run_time_so_far": 33, "deadline": 9000,
    },
    "Heartbeat": {
        "worker_id": 7,
        "job_state": [{"job_id": 4, "status": 2}],
    },
}


def dump(name, obj):
    """Compact JSON, one line per second-level entry."""
    path = os.path.join(OUT, name)
    enc = lambda o: json.dumps(o, separators=(",", ":"))
    with open(path, "w") as f:
        f.write("{\n")
        f.write(",\n".join(
            enc(k) + ":{\n" + ",\n".join(
                enc(k2) + ":" + enc(v2) for k2, v2 in v.items()
            ) + "\n}"
            for k, v in obj.items()
        ))
        f.write("\n}\n")
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


def run_lengths(seq):
    runs = []
    for x in seq:
        if runs and runs[-1][0] == int(x):
            runs[-1][1] += 1
        else:
            runs.append([int(x), 1])
    return runs


def load_oracle_functions(utils_py):
    ns = {}
    for node in ast.parse(open(utils_py).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name in (
            "get_gns_bs_pattern", "get_accordion_bs_pattern",
        ):
            exec(compile(ast.Module(body=[node], type_ignores=[]),
                         utils_py, "exec"), ns)
    return ns["get_gns_bs_pattern"], ns["get_accordion_bs_pattern"]


def load_result_pickle(path):
    class _JobIdPair:
        def __init__(self, *a, **k):
            pass

        def __hash__(self):
            return hash((self.__dict__.get("_job0"),
                         self.__dict__.get("_job1")))

        def __eq__(self, o):
            return isinstance(o, _JobIdPair) and self.__dict__ == o.__dict__

    class Unpickler(pickle.Unpickler):
        def find_class(self, module, name):
            if module == "job_id_pair" and name == "JobIdPair":
                return _JobIdPair
            return super().find_class(module, name)

    with open(path, "rb") as f:
        return Unpickler(f).load()


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--reference", required=True,
                   help="root of a reference checkout (holds scheduler/)")
    args = p.parse_args()
    sched = os.path.join(args.reference, "scheduler")
    os.makedirs(OUT, exist_ok=True)

    # -- on-disk inputs, verbatim / re-serialized
    shutil.copyfile(
        os.path.join(sched, "traces", "reproduce", TRACE_NAME + ".trace"),
        os.path.join(OUT, "trace_120.trace"),
    )
    shutil.copyfile(
        os.path.join(sched, "configurations", "tacc_32gpus.json"),
        os.path.join(OUT, "tacc_32gpus.json"),
    )
    oracle = json.load(open(os.path.join(sched, "tacc_throughputs.json")))
    dump("tacc_throughputs.json", {
        "v100": {k: {"null": v["null"]} for k, v in oracle["v100"].items()},
    })

    # -- committed simulation results
    sims = {}
    for policy in SIM_POLICIES:
        r = load_result_pickle(os.path.join(
            sched, "reproduce", "pickles", "tacc_32gpus",
            f"{policy}_{TRACE_NAME}_simulation.pickle",
        ))
        sims[policy] = {
            "makespan": float(r["makespan"]),
            "avg_jct": float(r["avg_jct"]),
            "finish_time_fairness_list": [
                float(x) for x in r["finish_time_fairness_list"]
            ],
        }
    dump("sim_results.json", sims)

    # -- batch-size oracle outputs
    from shockwave_amd.core import bs_patterns as bp

    ref_gns, ref_acc = load_oracle_functions(os.path.join(sched, "utils.py"))
    gns = {}
    for key in json.load(open(os.path.join(
            os.path.dirname(bp.__file__), "data", "gns_bs_ladder.json"))):
        model, bs, sf = key.split("|")
        jt = f"{model} (batch size {bs})"
        gns[key] = {
            str(E): run_lengths(ref_gns(jt, int(bs), E, int(sf)))
            for E in GNS_EPOCHS
        }
    acc = {}
    for model, bs in ACCORDION_COMBOS:
        jt = f"{model} (batch size {bs})"
        acc[f"{model}|{bs}"] = {
            str(E): run_lengths(ref_acc(jt, bs, E, 1))
            for E in ACCORDION_EPOCHS
        }
    dump("bs_patterns.json", {"gns": gns, "accordion": acc})

    # -- protobuf schema facts and wire bytes
    from shockwave_amd.rpc.pb import Schema

    ref = Schema(os.path.join(sched, "runtime", "protobuf"), "reference")
    dump("proto_fields.json", {
        "messages": {
            name: sorted(
                [f.name, f.number, bool(f.is_repeated)]
                for f in cls.DESCRIPTOR.fields
            )
            for name, cls in sorted(ref.messages.items())
        },
        "enums": {k: dict(v) for k, v in sorted(ref.enums.items())},
    })
    wire = {}
    for name, payload in WIRE_PAYLOADS.items():
        msg = ref.to_message(name, payload)
        back = ref.messages[name]()
        back.ParseFromString(msg.SerializeToString())
        wire[name] = {
            "payload": payload,
            "hex": msg.SerializeToString().hex(),
            "decoded": ref.to_dict(back),
        }
    dump("wire_messages.json", wire)


if __name__ == "__main__":
    main()
