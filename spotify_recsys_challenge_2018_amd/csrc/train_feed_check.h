// train_feed_check.h -- the host-side validation of dae_train_set_create (train_feed.hip), free of HIP so that a plain C++
// program can exercise it (tests/host/train_set_check_main.cpp).  The device path relies on what is checked here: offsets
// that start at 0 and never descend, every track in [0, n_tracks), every artist in [n_tracks, n_items) -- dae_train_batch
// carries no per-entry range flag.  Likewise dae_train_set_attach_titles' check of the title rows, further down.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

struct dae_train_set_shape {
    int64_t n_trk = 0, n_art = 0;      // entries of the two id arrays (trk_off[n_playlists], art_off[n_playlists])
    int max_side = 0;                  // longest single side of a playlist
    int max_row = 0;                   // longest playlist, tracks + artists
};

// 0 = the table is well formed (`shape` filled in); otherwise the DAE_ERR_* code to return, with the reason in `msg`
inline int dae_train_set_check(const int32_t* trk, const int64_t* trk_off, const int32_t* art, const int64_t* art_off,
                               int n_playlists, int n_tracks, int n_items, dae_train_set_shape* shape, char* msg,
                               size_t msg_len)
{
    constexpr int ERR_ARG = -1;        // DAE_ERR_ARG (include/dae_hip.h)
    if (!trk_off || !art_off || !shape || !msg) {
        if (msg) snprintf(msg, msg_len, "null pointer");
        return ERR_ARG;
    }
    if (n_playlists < 1 || n_tracks < 1 || n_items < n_tracks) {
        snprintf(msg, msg_len, "bad shape: %d playlists, %d tracks, %d items", n_playlists, n_tracks, n_items);
        return ERR_ARG;
    }
    const int64_t* offs[2] = {trk_off, art_off};
    const char* names[2] = {"trk_off", "art_off"};
    int64_t total[2] = {0, 0};
    int max_side = 0;
    int64_t max_row = 0;
    for (int s = 0; s < 2; ++s) {
        if (offs[s][0] != 0) {
            snprintf(msg, msg_len, "%s[0] = %lld, must be 0", names[s], (long long)offs[s][0]);
            return ERR_ARG;
        }
        for (int p = 0; p < n_playlists; ++p) {
            const int64_t a = offs[s][p], b = offs[s][p + 1];
            if (b < a || b - a > INT32_MAX / 2) {
                snprintf(msg, msg_len, "%s[%d] = %lld -> %lld: offsets must ascend, a side holds < 2^30 entries", names[s], p,
                         (long long)a, (long long)b);
                return ERR_ARG;
            }
            if ((int)(b - a) > max_side) max_side = (int)(b - a);
        }
        total[s] = offs[s][n_playlists];
    }
    for (int p = 0; p < n_playlists; ++p) {
        const int64_t len = (trk_off[p + 1] - trk_off[p]) + (art_off[p + 1] - art_off[p]);
        if (len > max_row) max_row = len;
    }
    if ((total[0] > 0 && !trk) || (total[1] > 0 && !art)) {
        snprintf(msg, msg_len, "null pointer");
        return ERR_ARG;
    }
    for (int64_t i = 0; i < total[0]; ++i)
        if (trk[i] < 0 || trk[i] >= n_tracks) {
            snprintf(msg, msg_len, "trk[%lld] = %d is no track id: tracks lie in [0, %d)", (long long)i, trk[i], n_tracks);
            return ERR_ARG;
        }
    for (int64_t i = 0; i < total[1]; ++i)
        if (art[i] < n_tracks || art[i] >= n_items) {
            snprintf(msg, msg_len, "art[%lld] = %d is no artist id: artists lie in [%d, %d)", (long long)i, art[i], n_tracks,
                     n_items);
            return ERR_ARG;
        }
    shape->n_trk = total[0];
    shape->n_art = total[1];
    shape->max_side = max_side;
    shape->max_row = (int)max_row;
    return 0;
}

constexpr int DAE_TRAIN_TITLE_MAX_LEN = 64;     // csrc/title.hip T_MAX_LEN: the longest title the title kernels take

// dae_train_set_attach_titles' validation (tests/host/train_titles_check_main.cpp): titles [n_playlists][L], every entry -1
// (no character) or a character id in [0, n_char).  `set_playlists`: the playlists of the set the titles join.
// 0 = well formed; otherwise the DAE_ERR_* code to return, with the reason in `msg`.  dae_train_titles copies rows as they
// are: it carries no per-entry check either.
inline int dae_train_titles_check(const int32_t* titles, int n_playlists, int set_playlists, int L, int n_char, char* msg,
                                  size_t msg_len)
{
    constexpr int ERR_ARG = -1;        // DAE_ERR_ARG (include/dae_hip.h)
    if (!titles || !msg) {
        if (msg) snprintf(msg, msg_len, "null pointer");
        return ERR_ARG;
    }
    if (n_playlists < 1 || n_playlists != set_playlists) {
        snprintf(msg, msg_len, "titles of %d playlists for a set of %d", n_playlists, set_playlists);
        return ERR_ARG;
    }
    if (L < 1 || L > DAE_TRAIN_TITLE_MAX_LEN) {
        snprintf(msg, msg_len, "title length %d: must be in [1, %d]", L, DAE_TRAIN_TITLE_MAX_LEN);
        return ERR_ARG;
    }
    if (n_char < 1) {
        snprintf(msg, msg_len, "n_char = %d: must be at least 1", n_char);
        return ERR_ARG;
    }
    for (int p = 0; p < n_playlists; ++p)
        for (int i = 0; i < L; ++i) {
            const int32_t c = titles[(size_t)p * (size_t)L + i];
            if (c < -1 || c >= n_char) {
                snprintf(msg, msg_len, "titles[%d][%d] = %d is no character: -1 (none) or an id in [0, %d)", p, i, c, n_char);
                return ERR_ARG;
            }
        }
    return 0;
}
