"""The names illico_ctx_set_option accepts, read out of the one table that declares them (illico_amd/csrc/options.h)."""
import re

from conftest import ROOT


def engine_option_names():
    """One OPT_*(name...) line per option after `kEngineOptions[] = {`, in the table's order."""
    src = (ROOT / "illico_amd" / "csrc" / "options.h").read_text()
    table = src[src.index("kEngineOptions[] = {"):]
    return re.findall(r"^\s*OPT_[A-Z0-9_]+\((\w+)", table[:table.index("};")], re.M)
