#!/usr/bin/env python3
"""Regenerates tests/golden/sql_pin.json: digests of the two ClickHouse statements that tests/test_sql_pin.py quotes
(compose/clickhouse/create.sh:64-68 flows_raw_view, :92-110 flows_5m_view), taken from a checkout of the reference.
The test compares its quoted text against these digests, so it needs no copy of the reference to run.

    python tests/golden/make_sql_pin.py <path of a flow-pipeline checkout>
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = "compose/clickhouse/create.sh"
STATEMENTS = {"flows_raw_view": (64, 68), "flows_5m_view": (92, 110)}  # 1-based, inclusive


def squash(s):
    """Whitespace-insensitive form of a statement (the test applies the same)."""
    return " ".join(s.split())


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    raw = open(os.path.join(sys.argv[1], SOURCE), "rb").read()
    lines = raw.decode().split("\n")
    out = {"source": SOURCE, "source_sha256": hashlib.sha256(raw).hexdigest(), "statements": {}}
    for name, (first, last) in STATEMENTS.items():
        text = squash("\n".join(lines[first - 1:last]))
        assert text.startswith("CREATE MATERIALIZED VIEW IF NOT EXISTS %s " % name), (name, text[:80])
        out["statements"][name] = {"lines": [first, last], "squashed_sha256": hashlib.sha256(text.encode()).hexdigest()}
    with open(os.path.join(HERE, "sql_pin.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
