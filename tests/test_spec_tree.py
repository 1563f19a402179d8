"""The tree drafter of GPTConfig::speculateTree (tinygpt_amd/host/spec_draft.h ngram_tree) without a GPU: tests/spec_tree_check.cpp, a stand-alone program under
the address and undefined-behaviour sanitizers — scripted cases (the most recent occurrence first, distinct first continuations only, the budget's split, more
candidates than nodes) and random sequences against the definition spelled out: topological order, distinct siblings, at most max_nodes nodes and max_branches
chains, the most recent occurrence first, and the first chain exactly ngram_draft cut to its share of the budget — properties, not a second implementation."""
import subprocess

from tinygpt_amd import build


def test_spec_tree_check():
    exe = build.build_spec_tree_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert "spec_tree_check: ok" in r.stdout
