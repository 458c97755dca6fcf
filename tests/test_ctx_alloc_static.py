"""The context's device memory has ONE owner (mimsem_amd/csrc/ctx.hpp: mimsem_ctx::alloc / release / owned): a table added to mimsem_ctx
is freed with the context, counted in mimsem_ctx_workspace_bytes and kept alive for the recordings that hold its address without being
named anywhere else.  These checks read the sources: nothing under csrc/ allocates or frees device memory outside the owner's routines,
except the short list below of memory that is NOT the context's (a handle's own, or a temporary its function frees before it returns);
and the two hand-kept lists the owner replaced stay gone."""
import pathlib
import re

CSRC = pathlib.Path(__file__).resolve().parents[1] / "mimsem_amd" / "csrc"
CALLS = re.compile(r"\b(hipMalloc\w*|hipExtMalloc\w*|hipFree(?:Async)?)\s*\($")      # (pinned host memory, hipHostMalloc / hipHostFree, is not meant)
OWNER = {("api.hip", "mimsem_ctx::alloc"), ("api.hip", "mimsem_ctx::release"), ("api.hip", "mimsem_ctx_destroy")}
ALLOWED = {
    ("api.hip", "mimsem_malloc"), ("api.hip", "mimsem_free"),                        # the caller's own vectors
    ("api.hip", "stamps_begin"),                                                     # stamps of the diagnostic build (MIMSEM_STAMPS)
    ("api.hip", "mimsem_block_inverse_status"),                                      # d_err: freed before it returns
    ("column_kernels.hip", "mimsem_selftest_rows_half"),                             # dE: likewise
    ("owned_blocks.hip", "mimsem_owned_blocks_build"),                               # em: likewise
    ("ksp.hip", "ensure"), ("ksp.hip", "mimsem_ksp_destroy"),                        # a mimsem_ksp's workspace and preconditioners
    ("ksp.hip", "zero_form_jacobi"), ("ksp.hip", "mimsem_ksp_set_pc_bjacobi"),       #   (and the temporaries of their builders)
    ("ksp.hip", "mimsem_ksp_set_pc_bjacobi_owned"), ("ksp.hip", "mimsem_ksp_set_pc_sw_bjacobi"),
    ("halo.hip", "mimsem_halo_create"), ("halo.hip", "mimsem_halo_destroy"), ("halo.hip", "mimsem_halo_peer_export"),   # a halo handle's buffers
}
NAME = re.compile(r"([\w:~]+)\s*\((?:[^()]|\([^()]*\))*\)\s*(?:const\s*)?$")


def _sites():
    """(file, enclosing function, line) of every device allocation or free under csrc/.  A small scan by brace depth: the enclosing
    function is the outermost `name(...) {` around the call (namespace, extern "C" and struct blocks end in no parenthesis)"""
    out = []
    for path in sorted(p for p in CSRC.iterdir() if p.suffix in (".hip", ".inc", ".hpp")):
        src = re.sub(r"//[^\n]*|\"(?:\\.|[^\"\\\n])*\"", "", path.read_text())          # comments and strings hold no code
        stack, stmt, line = [], "", 1                                              # stack: per open brace, the function it opens or None
        for i, ch in enumerate(src):
            if ch == "\n":
                line += 1
            if ch == "{":
                m = NAME.search(stmt.strip()) if not any(stack) else None
                stack.append(m.group(1) if m else None)
                stmt = ""
            elif ch == "}":
                if stack:
                    stack.pop()
                stmt = ""
            elif ch == ";" and not any(stack):
                stmt = ""
            else:
                stmt += ch
            if ch == "(" and CALLS.search(src[max(0, i - 40):i + 1]):
                out.append((path.name, next((f for f in stack if f), None), line))
    return out


def test_device_memory_is_allocated_and_freed_by_its_owner_only():
    sites = _sites()
    seen = {(f, fn) for f, fn, _ in sites}
    assert OWNER <= seen, "the owner's routines were not found: %s" % sorted(OWNER - seen)
    stray = [s for s in sites if (s[0], s[1]) not in OWNER | ALLOWED]
    assert not stray, "device memory allocated or freed outside mimsem_ctx::alloc / release: %s" % stray
    assert ALLOWED <= seen, "allow-list entries that no longer exist: %s" % sorted(ALLOWED - seen)


def test_no_hand_kept_list_of_the_context_s_buffers():
    text = {p.name: p.read_text() for p in CSRC.iterdir() if p.suffix in (".hip", ".inc", ".hpp")}
    for name, src in text.items():
        assert not re.search(r"\bretired\s*\.\s*push_back|->retired\b|\bretired;", src), "%s keeps a list of retired buffers" % name
    api = text["api.hip"]
    body = api[api.index("void mimsem_ctx_destroy(mimsem_ctx* c) {"):]
    body = body[:body.index("\n}\n")]
    assert not re.search(r"c->d_\w+", body), "mimsem_ctx_destroy names buffers one by one"
    assert "c->owned" in body
