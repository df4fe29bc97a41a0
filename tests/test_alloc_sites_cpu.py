"""CPU: every device and pinned allocation of the library goes through the context's allocator (csrc/ccal_internal.hpp: ctx_alloc /
ctx_release / ctx_cache_clear) - the cache, the record of live blocks and, through ctx_doubles / ctx_block_alloc / CallBlock, the test
hook's NaN fill all hang on that.  A source check: the four raw calls occur in csrc/ in that one header and nowhere else."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "camera_intrinsic_calibration_rs_amd", "csrc")
RAW = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\s*\(")


def test_raw_allocation_calls_only_in_the_allocator():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
    assert len(files) > 30 and os.path.join(CSRC, "ccal_internal.hpp") in files
    sites = {}
    for path in files:
        hits = [m.group(1) for m in RAW.finditer(open(path).read())]
        if hits:
            sites[os.path.basename(path)] = sorted(set(hits))
    assert sites == {"ccal_internal.hpp": ["hipFree", "hipHostFree", "hipHostMalloc", "hipMalloc"]}, sites
