"""Golden vector of SEG's ln(n!) table as the reference prints it (blast_seg.c:52-1308: `double lnfact[]`, 10 001 entries
with six decimals), parsed into float64 - the table test_seg_tables_pin.py compares the product's and the oracle's
derivations with, bit for bit.  Generated from the reference's source tree:
    python tests/golden/make_golden_lnfact.py <reference>/src/include/ncbi-blast+/algo/blast/core/blast_seg.c
Output (committed): tests/golden/seg_lnfact.npy."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

text = open(sys.argv[1]).read()
body = text[text.index("double lnfact[]"):]
body = body[body.index("{") + 1: body.index("};")]
printed = np.array([float(x) for x in re.findall(r"-?\d+\.\d+", body)], dtype=np.float64)
assert len(printed) == 10001, len(printed)
np.save(os.path.join(HERE, "seg_lnfact.npy"), printed)
