"""The demangled names of the forms of k_generate_candidate and k_temporal, built from keywords: the template parameter order of the
two kernels (frame_kernels.h; csrc/stage0_forms.h holds the forms the library instantiates) stands here once for the tools.

  generate_candidate(fuse=1, ws=1, raycast=1)                       'k_generate_candidate<true, false, false, false, true, true, false, false, false, false>'
  generate_candidate(fuse=1, ws=1, raycast=1, power=ANY, grid=ANY)  the same with (?P<power>true|false) and (?P<grid>true|false): a regular expression

A parameter that is not named is false, as the kernels' own defaults are. A name without ANY holds no character that is special in a
regular expression, so either result can be searched for with re or, without ANY, as plain text.
"""
GENERATE_CANDIDATE = ("fuse", "shadowed", "defer", "pipe", "ws", "raycast", "power", "reproject", "motion", "grid")
TEMPORAL = ("shadowed", "reproject", "motion")
ANY = object()  # either value, as a named group of the regular expression


def _form(kernel, order, given):
    unknown = set(given) - set(order)
    if unknown:
        raise TypeError("%s has no template parameter %s (it has %s)" % (kernel, ", ".join(sorted(unknown)), ", ".join(order)))
    args = ["(?P<%s>true|false)" % p if given.get(p) is ANY else ("true" if given.get(p) else "false") for p in order]
    return "%s<%s>" % (kernel, ", ".join(args))


def generate_candidate(**given):
    return _form("k_generate_candidate", GENERATE_CANDIDATE, given)


def temporal(**given):
    return _form("k_temporal", TEMPORAL, given)
