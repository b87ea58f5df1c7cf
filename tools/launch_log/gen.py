"""gen.py SFA_INTERNAL_H -- the logging stand-ins for the launchers that run.sh links against a tree's host code (printed to stdout, included by mock.cpp).
One body per declaration `void|bool|int launch_* | sor_* | run_grid_cut(...);` of the header: it logs the name and every argument; the launchers named in the
tuple below also call mock.cpp's special_<name>, which writes the norms and masks the host logic reads back.  The header is parsed with one regular expression:
a launcher declared in another shape (another return type, a body in the header) gets no stand-in, and run.sh then fails at its link step."""
import re, sys
hdr = open(sys.argv[1]).read()
hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
hdr = re.sub(r"//[^\n]*", "", hdr)
out = []
for m in re.finditer(r"\n(void|bool|int) ((?:launch_|sor_|run_grid_cut)\w*)\(([^;{]*?)\);", hdr):
    ret, name, params = m.groups()
    params = re.sub(r"\s+", " ", params)
    ps = [re.sub(r"\s*=\s*[^,]+$", "", p.strip()) for p in params.split(",")]
    names = [re.search(r"(\w+)(\[\d*\])?$", p).group(1) for p in ps]
    body = "    begin(\"%s\");\n" % name + "".join("    arg(\"%s\", %s);\n" % (n, n) for n in names if n != "c") + "    end();\n"
    body += "    special_%s(%s);\n" % (name, ", ".join(names)) if name in ("launch_set_mask", "launch_outer_threshold", "launch_update_inner", "launch_update_inner_x", "launch_update_outer_x", "launch_update_outer", "launch_exact_norms", "sor_operand_target") else ""
    body += {"void": "", "bool": "    return g_mock_bool;\n", "int": "    return SFA_OK;\n"}[ret]
    out.append("%s %s(%s) {\n%s}\n" % (ret, name, ", ".join(ps), body))
print("\n".join(out))
