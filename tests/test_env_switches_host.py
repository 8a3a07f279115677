"""
The TMVB_* environment switches of the library: one reader, one table.

csrc/ reads the environment only through the three helpers at the top of csrc/tmvb_internal.h (tmvb_env_on / tmvb_env_int, and tmvb_env_str for
the values that are text), and INTEGRATION.md section 4 has one table row per switch.  These tests hold the two together, keep a hand-written
getenv from coming back, and keep the switches that were retired -- each fixed at its default, with the kernels only they reached -- retired.
No GPU, no library: the sources and the document are read as text.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc")
INTEGRATION = os.path.join(ROOT, "INTEGRATION.md")

# retired: fixed at the default, the environment is no longer asked (TMVB_STREAM_POOL, once a candidate, is documented and stays)
REMOVED = {
    "TMVB_DEBUG_FLAGS", "TMVB_TS_CPL", "TMVB_CTPF_GRID_ANY", "TMVB_CTPF_SPLIT", "TMVB_CTPF_REG_ANY", "TMVB_CTPF_LONG_PRIO", "TMVB_CTPF_FUSE_STATS",
    "TMVB_CTPF_FUSED_MSTEP", "TMVB_CTM_FOLD_REDUCE", "TMVB_CTM_FORCE_GENERIC", "TMVB_CTM_MAX_TILE_KB", "TMVB_LDA_ELBO_LEGACY", "TMVB_LDA_ELBO_NO_PW",
    "TMVB_LDA_ELBO_EARLY", "TMVB_LDA_NO_LONG", "TMVB_LDA_PIECE_FRACS", "TMVB_LDA_CHAIN_AUX", "TMVB_LDA_SPLIT_OUT", "TMVB_LDA_ELBO_STREAM",
    "TMVB_LDA_SIDE_STREAM", "TMVB_CTPF_LONG_MERGE",
}
NAME = re.compile(r"TMVB_[A-Z0-9_]+")
READ = re.compile(r"\btmvb_env_(?:on|int|str)\(\s*\"(TMVB_[A-Z0-9_]+)\"")
HELPER = re.compile(r"^static inline [a-z* ]+ ?\*? ?tmvb_env_(?:on|int|str)\(")


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _names_read():
    return {n for p in _sources() for n in READ.findall(_read(p))}


def _table_rows():
    """rows of the switch table: | `TMVB_X` | default | read | what it selects | set by |"""
    rows = {}
    for line in _read(INTEGRATION).splitlines():
        m = re.match(r"^\| `(TMVB_[A-Z0-9_]+)` \|", line)
        if m:
            cells = [c.strip() for c in line.strip().strip("|").split("|")]
            assert m.group(1) not in rows, f"two rows for {m.group(1)}"
            rows[m.group(1)] = cells
    return rows


def test_every_switch_read_has_its_row_and_every_row_its_switch():
    read, rows = _names_read(), _table_rows()
    assert len(read) > 30                                        # the patterns still find the call sites
    assert read == set(rows), (sorted(read - set(rows)), sorted(set(rows) - read))
    for name, cells in rows.items():
        assert len(cells) == 5, (name, cells)
        assert cells[2] in ("once per process", "per model", "per call", "per communicator plan"), (name, cells[2])
        assert all(cells), (name, cells)
        # the last column names the test that sets the switch, and that test does set it
        if cells[4] != "diagnostic, no test":
            m = re.fullmatch(r"`(tests/test_[a-z0-9_]+\.py)`", cells[4])
            assert m, (name, cells[4])
            assert name in NAME.findall(_read(os.path.join(ROOT, m.group(1)))), (name, m.group(1))


def test_retired_switches_stay_retired():
    me = os.path.abspath(__file__)
    files = _sources() + glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True) + glob.glob(os.path.join(ROOT, "tools", "*.py")) + \
        glob.glob(os.path.join(ROOT, "tools", "*.sh")) + [os.path.join(ROOT, "bench.py"), INTEGRATION]
    assert len(files) > 60
    hits = [(os.path.relpath(p, ROOT), n) for p in files if os.path.abspath(p) != me for n in set(NAME.findall(_read(p))) & REMOVED]
    assert not hits, hits
    assert not (_names_read() & REMOVED)


def test_getenv_only_inside_the_helpers():
    sites = [(os.path.basename(p), i + 1, line.strip()) for p in _sources() for i, line in enumerate(_read(p).splitlines()) if "getenv(" in line]
    assert len(sites) == 3, sites
    for unit, _, line in sites:
        assert unit == "tmvb_internal.h" and HELPER.match(line), (unit, line)
    # ... and the helpers are what the call sites use: nothing else wraps them
    assert {m for _, _, line in sites for m in re.findall(r"tmvb_env_(on|int|str)\(", line)} == {"on", "int", "str"}
