"""The sizes of the caller-owned buffers are part of what a layout refactor must not move: tools/workspace_table.py prints every
size query of the native library over a fixed grid (and the one layout offset the ABI exposes), and this test compares that table
with the committed copy, tests/golden/workspace_bytes.json.

The sizes of fc_radius_workspace_bytes, fc_graph_workspace_bytes and fc_precomp_workspace_bytes contain the scratch size hipcub
states for its scan, so a ROCm / rocPRIM upgrade can move those rows with no layout change here; then regenerate as well.

When a layout is changed ON PURPOSE, regenerate the copy and review its diff:

    python tools/workspace_table.py --json tests/golden/workspace_bytes.json
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'workspace_bytes.json')


def test_workspace_sizes_match_the_committed_table(tmp_path):
    out = tmp_path / 'table.json'
    # its own process: the tool hides the devices before the library loads, so the table is the same with and without a GPU
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'workspace_table.py'), '--json', str(out)], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    with open(out) as f:
        table = json.load(f)
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(table) == len(golden)
    moved = [(g, t) for g, t in zip(golden, table) if g != t]
    assert not moved, 'first differences (committed, now): %s' % moved[:10]
