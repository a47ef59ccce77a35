// Stand-alone program (no device, no HIP): the host-side validation of dae_train_set_attach_titles,
// csrc/train_feed_check.h dae_train_titles_check -- valid rows, the character range and the shape limits.  Exits 0 and
// prints "all checks passed" when each case gives the expected code and message.  Meant to be built with
// -fsanitize=address,undefined as well: the rows are a heap block of exactly n_playlists x L entries, so a read past
// them is caught.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "train_feed_check.h"

namespace {

int g_failed = 0;
constexpr int N_CHAR = 41;

// three playlists of L characters: a right-padded title, an empty one (all -1), a full one that reaches n_char - 1
std::vector<int32_t> good(int L)
{
    std::vector<int32_t> t((size_t)3 * L, -1);
    for (int i = 0; i < L; ++i) {
        if (i < (L + 1) / 2) t[i] = i % N_CHAR;
        t[(size_t)2 * L + i] = N_CHAR - 1 - i % N_CHAR;
    }
    return t;
}

void expect(const char* what, const std::vector<int32_t>& rows, int n_playlists, int set_playlists, int L, int n_char,
            int want_rc, const char* want_in_msg)
{
    std::vector<int32_t> t(rows);      // an exact-size heap copy: the sanitizer sees every byte the check may touch
    char msg[256] = "";
    const int rc = dae_train_titles_check(t.empty() ? nullptr : t.data(), n_playlists, set_playlists, L, n_char, msg, sizeof(msg));
    const bool ok = rc == want_rc && (!want_in_msg || strstr(msg, want_in_msg));
    printf("%-44s rc=%d %s%s\n", what, rc, msg, ok ? "" : "   <-- UNEXPECTED");
    if (!ok) ++g_failed;
}

}  // namespace

int main()
{
    expect("valid rows, L = 25", good(25), 3, 3, 25, N_CHAR, 0, nullptr);
    expect("valid rows, L = 1", good(1), 3, 3, 1, N_CHAR, 0, nullptr);
    expect("valid rows, L = 64 (the limit)", good(64), 3, 3, 64, N_CHAR, 0, nullptr);
    { auto t = good(25); t[2 * 25 + 24] = N_CHAR; expect("character id == n_char (last entry)", t, 3, 3, 25, N_CHAR, -1, "titles[2][24] = 41 is no character"); }
    { auto t = good(25); t[0] = N_CHAR; expect("character id == n_char (first entry)", t, 3, 3, 25, N_CHAR, -1, "titles[0][0] = 41 is no character"); }
    { auto t = good(25); t[25 + 3] = -2; expect("character id -2", t, 3, 3, 25, N_CHAR, -1, "titles[1][3] = -2 is no character"); }
    { auto t = good(25); t[7] = INT32_MIN; expect("character id INT32_MIN", t, 3, 3, 25, N_CHAR, -1, "titles[0][7]"); }
    // L = 0 and L past the limit are refused before a single entry is read: the block holds nothing that long
    expect("L = 0", good(1), 3, 3, 0, N_CHAR, -1, "title length 0");
    expect("L = 65", good(1), 3, 3, 65, N_CHAR, -1, "title length 65");
    expect("L negative", good(1), 3, 3, -5, N_CHAR, -1, "title length -5");
    expect("titles of another number of playlists", good(25), 3, 4, 25, N_CHAR, -1, "titles of 3 playlists for a set of 4");
    expect("no playlists", good(25), 0, 0, 25, N_CHAR, -1, "titles of 0 playlists");
    expect("n_char = 0", good(25), 3, 3, 25, 0, -1, "n_char = 0");
    expect("null rows", std::vector<int32_t>(), 3, 3, 25, N_CHAR, -1, "null pointer");
    {
        char msg[8] = "";              // a short message buffer is respected
        auto t = good(25); t[0] = N_CHAR;
        const int rc = dae_train_titles_check(t.data(), 3, 3, 25, N_CHAR, msg, sizeof(msg));
        printf("%-44s rc=%d '%s'\n", "8-byte message buffer", rc, msg);
        if (rc != -1 || strlen(msg) != 7) ++g_failed;
    }
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
