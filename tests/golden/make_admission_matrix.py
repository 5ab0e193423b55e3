"""Records tests/golden/admission_matrix.json: the return code of every entry point on every kind of handle
(tests/admission_cases.py), on the GPU, at the commit whose behaviour is to be pinned.  Not a test.

    python tests/golden/make_admission_matrix.py <git hash of that commit> [output file]
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "vectordb-retrieval_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))


def main(recorded_at, out):
    import admission_cases as ac
    import vdbhip

    cells = {}
    for state in ac.STATES:
        report = {}
        cells[state] = ac.run_state(vdbhip, state, report)
        print(state, len(cells[state]), "cells", report, flush=True)
        if report["no_message"] or report["changed"]:
            raise SystemExit(f"{state}: a refused call left no message or changed the handle: {report}")
    Path(out).write_text(json.dumps({"recorded_at": recorded_at, "cells": cells}, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else str(ROOT / "tests" / "golden" / "admission_matrix.json"))
