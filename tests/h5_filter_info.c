/* Prints a dataset's shape, chunk shape, element size and signedness, and its filter pipeline (id, flags, cd_values):
 *   h5_filter_info FILE DATASET  ->  "rows cols chunk_rows chunk_cols size sign nfilters | id flags ncd cd..." */
#include <hdf5.h>
#include <stdio.h>

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    hid_t f = H5Fopen(argv[1], H5F_ACC_RDONLY, H5P_DEFAULT);
    if (f < 0) return 1;
    hid_t d = H5Dopen2(f, argv[2], H5P_DEFAULT);
    if (d < 0) return 1;
    hid_t sp = H5Dget_space(d), pl = H5Dget_create_plist(d), ty = H5Dget_type(d);
    hsize_t dims[2] = {0, 0}, chunk[2] = {0, 0};
    if (H5Sget_simple_extent_dims(sp, dims, NULL) != 2 || H5Pget_chunk(pl, 2, chunk) != 2) return 1;
    const int nf = H5Pget_nfilters(pl);
    printf("%llu %llu %llu %llu %zu %d %d", (unsigned long long)dims[0], (unsigned long long)dims[1], (unsigned long long)chunk[0],
           (unsigned long long)chunk[1], H5Tget_size(ty), (int)H5Tget_sign(ty), nf);
    for (int i = 0; i < nf; ++i) {
        unsigned flags = 0, cd[128], cfg = 0;
        size_t ncd = 128;
        char name[64];
        const H5Z_filter_t id = H5Pget_filter2(pl, (unsigned)i, &flags, &ncd, cd, sizeof name, name, &cfg);
        printf(" | %d %u %zu", (int)id, flags, ncd);
        for (size_t j = 0; j < ncd; ++j) printf(" %u", cd[j]);
    }
    printf("\n");
    H5Tclose(ty); H5Pclose(pl); H5Sclose(sp); H5Dclose(d); H5Fclose(f);
    return 0;
}
