"""The converter's branch model, the rate-pair grid, the bit-pattern comparison and the CAF / WAV writers of the
front-end tests: tools/converter_paths.py (shared with tools/fuzz_files.py, which must run without tests/), under the
name the tests import."""
import os
import sys

_TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)

from converter_paths import *  # noqa: E402,F401,F403
