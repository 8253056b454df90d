"""The kernel sources carry no compile-time switches besides the profiling hooks their tools build with: every preprocessor
conditional (#if, #ifdef, #ifndef, #elif, defined(...)) in csrc/*.hip, *.h and *.inc may name only identifiers of ALLOWED.  A
concluded experiment is deleted, not parked behind a -D: the live path is the only path a reader finds.  Reads source text only."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgb-no-more_amd", "csrc")
# hook -> the tool under tools/ that builds with it (through RGBNM_HIPCC_FLAGS); *_BLK: the encoder block the stamps are taken in
ALLOWED = {
    "CHAIN_PROF", "CHAIN_PROF_BLK",      # chain_prof.py
    "CHAINB_PROF", "CHAINB_PROF_BLK",    # chainb_prof.py
    "KP_PROF",                           # kpipe_prof.py
    "WRES_PROF",                         # wres_prof.py
    "WIN_PROF",                          # winattn_prof.py
    "AUG_PROF",                          # aug_prof.py
    "ATTN_PROF",                         # attn_prof.py
    "MLP_TRACE",                         # mlp_trace.py
}
DIRECTIVE = re.compile(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", re.M)


def conditional_names(text):
    """Identifiers that the conditionals of one source text test."""
    text = re.sub(r"\\\n", " ", text)                                  # continuation lines belong to their directive
    names = set(re.findall(r"\bdefined\s*\(\s*([A-Za-z_]\w*)\s*\)", text))
    for cond in DIRECTIVE.findall(text):
        cond = re.sub(r"//.*|/\*.*?\*/", "", cond)
        names |= set(re.findall(r"[A-Za-z_]\w*", cond)) - {"defined"}
    return names


def test_conditionals_name_only_the_profiling_hooks():
    files = sorted(f for ext in ("hip", "h", "inc") for f in glob.glob(os.path.join(CSRC, "*." + ext)))
    assert len(files) > 20
    seen = set()
    for f in files:
        names = conditional_names(open(f).read())
        assert names <= ALLOWED, f"{os.path.basename(f)} tests {sorted(names - ALLOWED)}: not a profiling hook"
        seen |= names
    assert seen == ALLOWED, f"allow-list entries no source tests any more: {sorted(ALLOWED - seen)}"


def test_the_scan_sees_every_form():
    src = "#ifdef X_A\n  #  if defined(X_B) && X_C == 2   // X_COMMENT\n#elif !defined X_D || \\\n    X_E\n#ifndef X_F\nint defined_x;\n"
    assert conditional_names(src) == {"X_A", "X_B", "X_C", "X_D", "X_E", "X_F"}
