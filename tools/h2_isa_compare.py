"""Are the kernels of two builds the same instructions?  Compares, function by function, two assembly files made with

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value --cuda-device-only -S \\
      grpc-rdma_amd/csrc/grdma_h2.hip -o NEW.s          (and the same at the commit to compare with -> OLD.s)
  python tools/h2_isa_compare.py OLD.s NEW.s [v]

after taking out what depends on a function's position in the file (the index in block labels, column padding).
Prints same / DIFF / only-old / only-new per function; with a third argument the first differing lines too.  This is
how k_h2_frame_one, k_h2_deframe and the chunk kernels were checked to be unchanged when k_h2_frame_links and
k_h2_deframe_links came to share their bodies (csrc/grdma_h2_frame_group.inc says which forms of sharing changed
k_h2_frame_one)."""
import re, sys, difflib
def funcs(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = cur; cur = None
            else:
                cur.append(re.sub(r"\s+", " ", re.sub(r"BB\d+_", "BB_", line)))  # (block labels carry the function's index in the file)
    return out
if __name__ == "__main__":
    a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
    for k in sorted(set(a) | set(b)):
        st = "only-old" if k not in b else "only-new" if k not in a else ("same" if a[k] == b[k] else "DIFF")
        print(st, k[:60], len(a.get(k, [])), len(b.get(k, [])))
        if st == "DIFF" and len(sys.argv) > 3:
            d = [l for l in difflib.unified_diff(a[k], b[k], n=0) if not l.startswith(("---", "+++"))]
            print("".join(d[:60]))
