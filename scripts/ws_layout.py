"""Where the regions of a tokenize / screened-search workspace are, in int32 words of the tensor the Python side keeps
(model._tok_ws): a restatement of `struct LqWorkspace` in lipvq-vae_amd/csrc/lipvq_screen.h for the measurement scripts -- change
the two together.  [64 B header][row list][best-candidate list][short lists][slot-2 list]..."""

HEADER = 16                    # kHeaderBytes / 4; [0] rows left to an exact decision, [1] listed rows, [8..10] the live counters


def list_ints(N):              # LqWorkspace::list_ints
    return (N + 15) & ~15


def short_cap(N):              # LqWorkspace::short_cap: slots that get a short list of 16 ints
    return N + 64


def row_list(N):
    return HEADER


def best_list(N):
    return HEADER + list_ints(N)


def short_lists(N):
    return HEADER + 2 * list_ints(N)


def slot2_list(N):
    return short_lists(N) + 16 * short_cap(N)


def stamps(N):                 # LqWorkspace::stamps (-DLQ_STAMPS builds): 16 int64 (32 words) per wave of the fused launch
    return HEADER + ((N // 2) & ~1)
