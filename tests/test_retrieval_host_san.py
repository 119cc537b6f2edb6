"""CPU: the host code of the retrieval-evaluation entry points (tvc_rank.cpp: slot checks, refusals, workspaces; the plan of
host_plan.hpp) runs clean under AddressSanitizer / UBSan with leak detection, as a stand-alone program
(tests/host_san_rank/driver.cpp on tests/host_san's HIP stand-in, built and run by tests/host_san_build.py)."""
import host_san_build


def test_rank_host_code_under_address_and_ub_sanitizers(tmp_path_factory):
    host_san_build.run_driver("host_san_rank", "HOST_SAN_RANK_OK", tmp_path_factory)
