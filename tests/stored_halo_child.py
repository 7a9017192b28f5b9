"""Child process of tests/test_stored_gpu.py::test_forced_halo_load_is_bit_identical: with QUDA_AMD_FORCE_GAUGE_HALO=1 in the environment (read
once per process by the loader) the links are loaded unpartitioned and with partition mask 15, where the backward links of every x_d = 0 face
come from the packed ghost slice of the process' own last slice, and the raw images are compared bit for bit."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import oracle_api  # noqa: E402
import stored_ref as S  # noqa: E402


def main():
    assert os.environ.get("QUDA_AMD_FORCE_GAUGE_HALO") == "1"
    qa = importlib.import_module("quda-qkxtm-multigrid_amd")
    oracle = oracle_api.load()
    X = S.LATTICES["12x6x10x4"]
    gauge, _, _ = oracle.make_fields(list(X), seed=S.SEEDS["12x6x10x4"], antiperiodic_t=True, clover=False)
    Wh = S.host_blocks(gauge, X)
    qa.init(0)
    try:
        for prec, recon in ((4, 12), (2, 8)):
            images = []
            for mask in (0, 15):
                qa.lib().qudaAmdSetPartitionMask(mask)
                qa.load_gauge(gauge, qa.gauge_param(X, cuda_prec=prec, recon=recon))
                i = qa.gauge_raw_info(0)
                images.append(qa.raw_device_copy(i["data"], i["bytes"]))
            W, stored, rs = S.decode_links(images[1], i, X, True)
            S.check_links("forced halo %d/%d" % (prec, recon), W, stored, rs, Wh, X, prec, recon, True)
            if not np.array_equal(images[0], images[1]):
                print("DIFFERENT prec %d recon %d: %d bytes" % (prec, recon, int(np.sum(images[0] != images[1]))))
                return 1
            print("IDENTICAL prec %d recon %d, %d bytes" % (prec, recon, images[0].size))
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)
        qa.end()
    return 0


if __name__ == "__main__":
    sys.exit(main())
