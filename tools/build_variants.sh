#!/bin/bash
# Rebuild the library and its diagnostic stamps variant (run after any change to csrc/ or the
# header: a stale variant lacks symbols the binding table expects and fails to load).
set -e
cd "$(dirname "$0")/.."
python3 -c "import __graft_entry__ as g; g.build()"
python3 -c "from grace_amd.build import build; build(variant='stamps')"
