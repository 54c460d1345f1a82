"""plaid.gsea's host argument checks under AddressSanitizer and UBSan, in a stand-alone program on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gsea_argument_checks_are_clean_under_asan_and_ubsan():
    """`make host-asan-gsea` compiles api.cpp and multi.cpp with -fsanitize=address,undefined on the host side, links them
    with tools/host_asan/gsea_args_main.cpp (its own main; exactly sized buffers) and runs it: the score type, the le_len /
    le_idx pair and the older checks in the header's order, through plaidhip_gsea_scored and its _multi form.  Every call
    ends in a check or at the missing context, so no device is needed; any report aborts the program."""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "plaid_amd", "csrc"), "host-asan-gsea"], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "[host-asan-gsea] ok" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
