// Stand-alone program (no device, no HIP): the host-side validation of dae_train_set_create, csrc/train_feed_check.h --
// the range checks and every error path.  Exits 0 and prints "all checks passed" when each case gives the expected code
// and message.  Meant to be built with -fsanitize=address,undefined as well: the arrays are heap blocks of exactly the
// advertised size, so a read past an offset or id array is caught.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "train_feed_check.h"

namespace {

int g_failed = 0;

struct Table {
    std::vector<int32_t> trk, art;
    std::vector<int64_t> trk_off, art_off;
    int n_tracks = 1000, n_items = 1200;
    int n_playlists() const { return (int)trk_off.size() - 1; }
};

Table good()
{
    Table t;
    t.trk = {0, 5, 999, 5, 7};
    t.trk_off = {0, 3, 3, 5};
    t.art = {1000, 1199, 1000};
    t.art_off = {0, 0, 2, 3};
    return t;
}

int run(const Table& t, dae_train_set_shape* shape, char* msg, size_t len)
{
    // exact-size heap copies: the sanitizer sees every byte the check may touch
    std::vector<int32_t> trk(t.trk), art(t.art);
    std::vector<int64_t> to(t.trk_off), ao(t.art_off);
    return dae_train_set_check(trk.empty() ? nullptr : trk.data(), to.data(), art.empty() ? nullptr : art.data(), ao.data(),
                               t.n_playlists(), t.n_tracks, t.n_items, shape, msg, len);
}

void expect(const char* what, const Table& t, int want_rc, const char* want_in_msg)
{
    dae_train_set_shape shape;
    char msg[256] = "";
    const int rc = run(t, &shape, msg, sizeof(msg));
    const bool ok = rc == want_rc && (!want_in_msg || strstr(msg, want_in_msg));
    printf("%-44s rc=%d %s%s\n", what, rc, msg, ok ? "" : "   <-- UNEXPECTED");
    if (!ok) ++g_failed;
}

}  // namespace

int main()
{
    {
        Table t = good();
        dae_train_set_shape shape;
        char msg[256] = "";
        const int rc = run(t, &shape, msg, sizeof(msg));
        const bool ok = rc == 0 && shape.n_trk == 5 && shape.n_art == 3 && shape.max_side == 3 && shape.max_row == 3;
        printf("%-44s rc=%d n_trk=%lld n_art=%lld max_side=%d max_row=%d%s\n", "a well-formed table", rc, (long long)shape.n_trk,
               (long long)shape.n_art, shape.max_side, shape.max_row, ok ? "" : "   <-- UNEXPECTED");
        if (!ok) ++g_failed;
    }
    { Table t = good(); t.trk[2] = 1000; expect("track id == n_tracks", t, -1, "trk[2] = 1000 is no track id"); }
    { Table t = good(); t.trk[0] = -1; expect("negative track id", t, -1, "trk[0] = -1 is no track id"); }
    { Table t = good(); t.art[1] = 999; expect("artist id below n_tracks", t, -1, "art[1] = 999 is no artist id"); }
    { Table t = good(); t.art[2] = 1200; expect("artist id == n_items", t, -1, "art[2] = 1200 is no artist id"); }
    { Table t = good(); t.trk_off[0] = 1; expect("offsets do not start at 0", t, -1, "trk_off[0] = 1"); }
    { Table t = good(); t.art_off[2] = 0; t.art_off[1] = 1; expect("descending offsets", t, -1, "art_off[1]"); }
    { Table t = good(); t.n_items = 999; expect("n_items < n_tracks", t, -1, "bad shape"); }
    { Table t = good(); t.n_tracks = 0; expect("no tracks", t, -1, "bad shape"); }
    {
        Table t = good();
        t.trk.clear(); t.trk_off = {0, 0, 0, 0};
        expect("a table without any track", t, 0, nullptr);
    }
    {
        Table t = good();      // ids advertised by the offsets, but no array
        dae_train_set_shape shape;
        char msg[256] = "";
        const int rc = dae_train_set_check(nullptr, t.trk_off.data(), t.art.data(), t.art_off.data(), t.n_playlists(), t.n_tracks,
                                           t.n_items, &shape, msg, sizeof(msg));
        printf("%-44s rc=%d %s\n", "null id array", rc, msg);
        if (rc != -1 || !strstr(msg, "null pointer")) ++g_failed;
    }
    {
        char msg[8] = "";      // a short message buffer is respected
        Table t = good(); t.trk[2] = 1000;
        dae_train_set_shape shape;
        const int rc = run(t, &shape, msg, sizeof(msg));
        printf("%-44s rc=%d '%s'\n", "8-byte message buffer", rc, msg);
        if (rc != -1 || strlen(msg) != 7) ++g_failed;
    }
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
