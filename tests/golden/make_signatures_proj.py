"""Record the reference's signatures of `proj` and `world_to_cam` as data
(tests/golden/signatures_proj.json) for tests/test_covar_host.py, in the
format of make_signatures.py: per function its parameters as
[name, kind, default repr].  Names and defaults only.

Run in the build container only (needs /root/reference):

    python tests/golden/make_signatures_proj.py
"""

import inspect
import json
import os
import sys
import types

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["proj", "world_to_cam"]


def main():
    pkg = types.ModuleType("gsplat")
    pkg.__path__ = [os.path.join(REF, "gsplat")]
    sys.modules["gsplat"] = pkg
    from gsplat.cuda import _wrapper

    sigs = {}
    for n in NAMES:
        params = []
        for p in inspect.signature(getattr(_wrapper, n)).parameters.values():
            d = None if p.default is inspect.Parameter.empty else repr(p.default)
            params.append([p.name, p.kind.name, d])
        sigs[n] = {"module": "gsplat.cuda._wrapper", "params": params}
    path = os.path.join(HERE, "signatures_proj.json")
    with open(path, "w") as f:
        json.dump(sigs, f, indent=1, sort_keys=True)
    print(f"wrote {path}: {len(sigs)} functions")


if __name__ == "__main__":
    main()
