/* pbr_file.h -- the one whole-file reader of the host layer's ...File loaders (private to host/). */
#ifndef PBR_FILE_H
#define PBR_FILE_H

#include <stdio.h>
#include <stdlib.h>

/* the bytes of `filepath` (the caller frees them) and their count in *size, never 0; or NULL after one line on stderr in the name of
 * `fn`: "cannot open" for a NULL or unopenable path, "cannot read" for a failed seek / tell, an empty file or a short read */
static inline void* pbr_read_file(const char* fn, const char* filepath, size_t* size) {
    FILE* f = filepath ? fopen(filepath, "rb") : NULL;
    if (!f) { fprintf(stderr, "GPU-ERROR: %s: cannot open %s\n", fn, filepath ? filepath : "(null)"); return NULL; }
    void* buf = NULL;
    long n = -1;
    if (fseek(f, 0, SEEK_END) == 0) n = ftell(f);
    if (!(n > 0 && fseek(f, 0, SEEK_SET) == 0 && (buf = malloc((size_t)n)) != NULL && fread(buf, 1, (size_t)n, f) == (size_t)n)) {
        fprintf(stderr, "GPU-ERROR: %s: cannot read %s\n", fn, filepath);
        free(buf);
        buf = NULL;
    }
    fclose(f);
    *size = buf ? (size_t)n : 0;
    return buf;
}

#endif
