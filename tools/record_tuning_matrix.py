"""What rt_tuning, rt_tuning_get and rt_trace_mode ANSWER, for every key / value / mode that is worth asking: no kernel runs.

    python tools/record_tuning_matrix.py PRODUCT.so EXPERIMENTS.so > tests/golden/tuning_matrix.json

tests/golden/tuning_matrix.json holds the answers of the commit BEFORE rt_tuning became a table (the 29-arm chain and the switch;
docs/MEASUREMENT_LOG_r12.md section 2 says how they were taken); tests/test_gpu_parity.py::test_tuning_matrix replays it on the
libraries of the tree, entry for entry. Record it anew only from libraries whose answers are known to be the wanted ones, e.g. after
a key was added on purpose.

Per library, on ONE fresh 64 x 48 whole-frame context, in this order: the default of every key (rt_tuning_get), then for every key
and every value {rt_tuning's code, rt_tuning_get's code, the value it reports (0 where it failed)}, then rt_trace_mode's codes.
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KEYS = list(range(-1, 31)) + [99]
VALUES = list(range(-3, 10)) + [255, 256, 257, 2048, 163840, 163841, 2**31 - 1]
MODES = list(range(-1, 9))


def measure(lib_path):
    from cedec_2024_rt_amd import api

    r = api.Renderer(64, 48, lib_path=lib_path)

    def get(key):
        v = C.c_int(0)
        return [r.L.rt_tuning_get(r.h, key, C.byref(v)), v.value]

    out = {"defaults": [get(k) for k in KEYS]}
    out["tuning"] = [[[r.L.rt_tuning(r.h, k, v)] + get(k) for v in VALUES] for k in KEYS]
    out["trace_mode"] = [r.L.rt_trace_mode(r.h, m) for m in MODES]
    r.close()
    return out


def main():
    product, experiments = sys.argv[1:3]
    doc = {"keys": KEYS, "values": VALUES, "modes": MODES, "product": measure(product), "experiments": measure(experiments)}
    print(json.dumps(doc, separators=(",", ":")))


if __name__ == "__main__":
    main()
