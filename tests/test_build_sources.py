"""The build id covers every file libdk_rx.so is built from (CPU only)."""
import os

import __graft_entry__ as G


def test_csrc_files_are_the_build_lists():
    """Every file in demikernel_amd/csrc is named in SOURCES or HEADERS, and nothing else is: tree_build_id hashes
    those lists, so a header outside them could change the library without changing its id, and the stale-library
    check (conftest.py) would pass a library built from other text."""
    listed = G.SOURCES + G.HEADERS
    assert len(set(listed)) == len(listed)
    assert set(os.listdir(G.CSRC)) == set(listed)
