"""Dev: per-kernel resource table of the post-processing chains for two builds, without a GPU.

Compile a translation unit that includes the four post-processing headers (ucb_kernels.h, ucb_rgb_kernels.h, ucb_tsm_kernels.h,
sfw_kernels.h) and calls the four launchers, once per tree:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I<tree>/blindshadowremoval_amd/csrc --cuda-device-only -S \
          -Rpass-analysis=kernel-resource-usage -o <name>.s tu.hip 2> <name>.txt
then: python scratch/post_resource_table.py parent.txt parent.s change.txt change.s  ->  a markdown table on stdout: VGPRs, SGPRs,
LDS and scratch bytes per kernel of both builds, and whether the kernel's instruction stream (labels, comments and directives
dropped) is the same.  `renames` pairs a parent kernel with the templated kernel that serves it in the other build."""
import re
import subprocess
import sys

RENAMES = {  # parent name -> change name
    "ucb_rgb_ssim_kernel": "ssim_pair_kernel<UcbRgbScratch>", "ucb_tsm_ssim_kernel": "ssim_pair_kernel<UcbTsmScratch>",
    "ucb_ssim_finish_kernel": "ssim_finish_kernel<UcbScratch>", "ucb_rgb_ssim_finish_kernel": "ssim_finish_kernel<UcbRgbScratch>",
    "ucb_tsm_ssim_finish_kernel": "ssim_finish_kernel<UcbTsmScratch>",
}
FIELDS = (("VGPRs", "VGPRs"), ("SGPRs", "TotalSGPRs"), ("LDS", "LDS Size [bytes/block]"), ("scratch", "ScratchSize [bytes/lane]"))


def demangle(names):
    out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    short = []
    for d in out[:len(names)]:
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\(.*$", "", d).replace("bsr::", "")
        short.append(d)
    return short


def remarks(path):
    res, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(.+?): (\d+) \[", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    names = list(res)
    return dict(zip(demangle(names), (res[n] for n in names)))


def streams(path):
    """kernel -> its instructions, operands included, with local labels, comments and directives dropped"""
    res, cur, names = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = res.setdefault(m.group(1), [])
            names.append(m.group(1))
            continue
        if re.match(r"^\.Lfunc_end", line):
            cur = None
        s = line.split(";")[0].strip()
        if cur is None or not s or s.startswith(".") or s.endswith(":"):
            continue
        cur.append(re.sub(r"\.LBB\d+_\d+", ".L", s))
    return dict(zip(demangle(names), (res[n] for n in names)))


def main(pr, ps, cr, cs):
    a, b, sa, sb = remarks(pr), remarks(cr), streams(ps), streams(cs)
    print("| kernel | VGPRs | SGPRs | LDS bytes | scratch bytes | instructions | same stream |")
    print("|---|---|---|---|---|---|---|")
    for name in a:
        new = RENAMES.get(name, name)
        cell = lambda key: "%d" % a[name][key] if a[name][key] == b[new][key] else "%d -> %d" % (a[name][key], b[new][key])
        n0, n1 = len(sa[name]), len(sb[new])
        print("| %s | %s | %s | %s | %s | %s | %s |" % (name if new == name else "%s -> %s" % (name, new), cell(FIELDS[0][1]), cell(FIELDS[1][1]),
                                                  cell(FIELDS[2][1]), cell(FIELDS[3][1]), "%d" % n0 if n0 == n1 else "%d -> %d" % (n0, n1),
                                                  "yes" if sa[name] == sb[new] else "no"))
    extra = sorted(set(b) - {RENAMES.get(n, n) for n in a})
    if extra:
        print("\nonly in the second build: " + ", ".join(extra))


if __name__ == "__main__":
    main(*sys.argv[1:5])
