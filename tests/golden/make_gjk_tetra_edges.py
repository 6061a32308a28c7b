"""Golden GJK vectors for two statements of reduce_tetra (csrc/lsc_gjk.hpp) that none of the other GJK vectors reaches: the set_edge
fall-backs of the `nface == 1`, `nkeep == 2` arms -- `ki`: the origin's foot on plane(a, pi, pk) is kept by edge a-pk and rejected by edge
a-pi (the reference then keeps edge a-pk); `kj`: the same with pj, where it keeps edge a-pj.

The hulls below were found by random search against a host build of the header with a counter on each of the two statements (nothing of
that build is kept): float32-valued 6-point hulls, normal coordinates at scales 1e-3 .. 1 around an offset of the same scale, thin in z for
half of them, small-integer lattices for an eighth.  Of 50 million hulls 164 reached the first statement and 235 the second; 16 per statement
are kept, as the bits of their float32 coordinates.  The answers are those of the REFERENCE's own openGJK (built in-container into oracle/_ref by
oracle/Makefile), as in make_gjk_golden.py.

Run in the build container only:  python tests/golden/make_gjk_tetra_edges.py
Writes tests/golden/gjk_tetra_edges.npz: pts float32 [32][6][3], statement int32 [32] (0: the `ki` arm, 1: the `kj` arm), v, dist, nvrtx.
"""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from oracle import oracle as O  # noqa: E402

KI_ARM = [
    "390c1683 3ad5eeda 3ad0aff5 b96b7320 ba51e668 3af5059c ba46b8ec 3a73eb48 3a572bed ba83c0f3 babe580b 3b3ff040 3910a416 bb3b5806 3b677a77 bb203018 bab0aa4a 3a78b093",
    "40000000 c0000000 3f800000 40000000 bf800000 c0000000 00000000 bf800000 c0000000 80000000 bf800000 c0400000 40400000 80000000 c0800000 3f800000 c0400000 40400000",
    "ba8831d1 3ac1d1f5 3bbe968e bb5522d6 ba65c8b0 3b5ac8f0 bb8c1f42 bb964dc7 3c0e5582 bab3cebe 3b1efa1f bb087a6f bbc102b7 3b049501 3af99af9 ba313d3a 3a06d879 b94444a7",
    "bc078c98 3be1fdd5 3b1b8e70 bb32e17b 3aae069e 3a8b9c11 3b2acaad 3bfb4372 3bc5f03c bbfe7b48 ba0a659b bb84dc80 bac60d13 3b980d8f bbf2ebaf bb8ef8e9 b88026cb bb0a7c7c",
    "3b2b20c5 3ceba4fe 3be82126 3c53ad24 3c5c5d91 3c060eef 3d07d65a bb5e26ec bcca7b3a ba301a4c 3cb98c61 3d09a985 3d1b05d3 3c0d4dc9 3c3bf210 3c9dd6a2 3b93159d bb94c731",
    "be9e4bcf 3a54429c 3db10e96 bdb899f1 3de9284f 3e03ddf0 3c88e790 be21ab9a 3e31105d bdc25794 be2e8826 3cb61b8c be0a1b00 bf2ffd93 bd3f9988 be279105 bd541b15 3e9b2dde",
    "3b0c760a 3b38eb1d ba48e7c5 3b6762cd bbb80a77 bb4bb1a8 3b3eb4a0 bb96fc6c bb32a1a7 3bac3560 3b828ed7 bb89c581 3b871d40 bb11a936 bb3cadf3 ba5ab257 3bf49e79 ba821eaf",
    "3be9d33c 3b9a571f bcb9f64a 3b92c598 bbc03ed0 3addcd09 3c2c1f1a bc6e8e94 3b811723 3c058bef bc621550 3b40dad8 3c6f5696 3cf2ac6d bc6090d8 3bd47525 bc2a63b8 bbab9696",
    "be017312 3f206e45 bf904a5c 3d38648c 3f73775f 3f079292 3f82d1a6 3edfd008 bd254fa5 bf05be53 bd98cab3 be290910 3eeed34b 3e47c23c bccfa433 be6ab25e 3f5ce40a 3f01eadd",
    "bd4fc2bb bf39caef bf5b0e0a bf4cccc8 be943d51 beb94187 bf851248 bf2875ca bf11930f 3d63c204 bdf9d8d6 3dfcf80c 3f482b13 bf925254 bf296328 3eeae7fc bf2c21dc 3f48c58d",
    "3c2acbd0 3bab3946 bc351913 ba49e7c9 3b93a150 b8ec1f8f 3b438884 3bc08978 bb13ff53 bc5814a7 3c261f28 bb8f7e47 3c9da9e1 3ba2a28e 3bd54ad4 bbd0e02e 3c12b523 ba10cc2e",
    "b9885e86 b96e1a41 3a9856af 3b4dca10 ba26c283 ba35e5d8 baecddd8 b92dbc5b 3abe3590 3967a733 38083f2a 37abc3e4 3a2918d1 ba30e28b 3b11a8e3 baeab54f 3aac2605 3ac38de7",
    "3f0615f0 bcf34a18 3ed4d754 3e7b678d 3d39c507 3f656d74 3e926d92 3ebe19f5 be2680c1 3ee0483c 3e61e1c7 3ecfd620 3eca924d 3f055016 bead9e9b 3e7713f7 3ec26644 3e297744",
    "bdc409a6 bd634c7e bd36c122 3b28eb79 3e4c6c26 3c0a3c03 bd2b7928 3d5509f8 3d0c568f bd3fe3dc bccdb19b bd238fd6 3cf59830 bccaa1c2 bdcc6b23 bcc77760 3d02cbab 3c2eebe3",
    "3b2ea418 bb2464fa bc3fe292 3b9eb04d 3bb6508b bc3f2eca 3a8e8abe 3ab7089f bc3eee3b 3b540cfb bc5d6263 bc408b5b bb0a1816 bb17727b bc3ff183 3bb16398 3c17fd3e bc40defe",
    "bf800000 c0a00000 80000000 80000000 00000000 bf800000 c0000000 00000000 40000000 00000000 c0400000 bf800000 c0000000 c0000000 3f800000 3f800000 80000000 c0800000",
]

KJ_ARM = [
    "bae9dabb bbdfc2fe 3b21f477 bb888cd0 bb07ce99 3b32706f bbdca267 3b637ac5 3b2742cb 3c99c30c bc205839 3b2e3260 3b09315b ba90e90f 3b20c4b9 bb77fe72 3a9df449 3b20cf2d",
    "3d13ff39 3d40b5ba 3d5b759e bd08454e 3e089f7d bae4c517 bd8d34e3 3c6f2165 bc5dd894 3cf9af7d bbef48a7 3d636fad bd9369d9 3c91c03e 3cd86f43 3df765d1 bc8c5d81 3e10b5e1",
    "bb5f900d 3c727545 3a2f9568 bc7a052e 3b08fe77 3b294b50 3c01d645 3a13c6cd 3cc6cd17 bc392022 3b5b670a bc099722 bcf045c1 3c0f23d4 bcd256a8 bc147bd6 3ca3c43a 3c03c433",
    "3d2b187f bd00d0e4 bdda19fb 3c91631f bd396312 bdd89f59 3d08065b bd09eb7d bdd98529 ba416c7c 3c9f7a64 bdd8e00a bb6d7bfc bd876d76 bdd96ea7 bb9bb754 bd2a0f23 bdd74d25",
    "3b6a28b9 bb86e98c bbe956e0 3b8ca3a7 baacff5d bbe9e04a bc03cd73 bb53d50e bbe054ec bce92a02 bbcbf279 bbe9124d 3c987957 3b8eeebe bbe783c4 3c2a7daa 3b33d50c bbdd4f50",
    "3a5437a6 bb21546d bb6ac9e8 3aeefc99 3a750aa5 bac48dd7 bb396678 39f2bea3 ba65098e 39597a70 3af1ea7d bb9b2a2e 3bae8f73 3ae435a6 bb84e538 ba94cbbe 398a946c ba4fe13c",
    "b9d36ea0 ba6a9edf b9d7aeee 3b32fc7d ba57c752 bb8fda3c 39269146 b7821a60 ba0e20d5 bb0e3f60 3a298f6b bac0bfab baf90dfc bb09a213 3a09a765 baa2b113 39abbe66 3a4019e2",
    "ba0868e8 39d9b479 3babaedc 38cfbf01 3a0948c1 3bab1e39 3a8d9048 3b6e402b 3babe90e bb5efa36 bb352946 3bab8c0b bb28bbea 39e510d0 3baae969 b9becf8b ba68d34d 3bac58b1",
    "3f277cc7 bd59b758 3f3b54d1 3ee7adf9 3eee859b 3eaa1c1c bec5234c bf0cb54b 3fdd6383 bf7b8a3e 3e82a4f6 3f89c676 3f6a97a6 3f17ca1f 3e5c6bf8 3f25b92e 3cc5d151 3f4e3900",
    "3e0846af bbcaad85 3ecdb267 3f1f9771 3e9619e0 3e97bbbc 3e6834bf 3d4d7ae9 3ebd2a3d bdb12bec beb7d8f2 3d1ad27e 3f16dab7 3e5060b3 3d9f3637 3e7c47bd 3da33c7e 3cef8ee6",
    "3f800000 3f800000 40000000 bf800000 bf800000 40000000 80000000 bf800000 40000000 c0000000 40400000 bf800000 3f800000 c0400000 40800000 bf800000 3f800000 40000000",
    "bb8619ff 3b52a1c0 ba4bc8c3 bb7ebe92 39c25ba4 bb6beec1 bb969d52 ba56a858 bc0b8735 38f8d01b 3ba4bcf5 3a40405b 394ac786 bc144bf9 bb61be4b 39338d5b 3c2ffd32 3ae6b160",
    "bb855d6a b9ebfdef 3b744c04 baecd10d 389ee895 ba9f1a18 ba050989 3b03cd25 b951086d bbe5a8e1 bb81b264 bb2b4984 bb326833 bab28dad ba97d54b bbb5d508 3b970343 bb9669f4",
    "bf24513a 3f0a58e8 3c742640 be313b98 be174731 3e8c56bc bf7c76ac 3e263344 bf1a6c38 bf9c8658 3e895cc9 3f5e51b7 be975c68 bd872b0a bee6b9be bf41be09 bdb5ad21 bfbe74b7",
    "3c91b04a 3be9370b bc39146d 3bf81311 bcbbefb7 bc32a4b0 3c190c3f 3b77460a bcb32531 3c5b7aaf 3be4c4f5 3c11af9e 3cda4d5f 3ca985d9 3caeaf46 3bff3be7 3a8c7151 bcd51a2c",
    "bf8342e0 bf92b82c bf02836d 3cf41993 bed50dd0 3eb8f00e bee8fa23 3ef6ca1f bfc1c179 3eaa26d7 be5b4eb8 beeb0b4e be409d2f bfe74bc0 3fa2417a bf28340c bf6355e7 3d17335d",
]


def hulls():
    """(pts float32 [32][6][3], statement int32 [32])."""
    rows = KI_ARM + KJ_ARM
    bits = np.array([[int(w, 16) for w in r.split()] for r in rows], np.uint32)
    return bits.view(np.float32).reshape(len(rows), 6, 3), np.array([0] * len(KI_ARM) + [1] * len(KJ_ARM), np.int32)


def main():
    ref = O.ref_gjk_lib()
    if ref is None:
        raise SystemExit("oracle/_ref/libref_opengjk.so missing: run `make -C oracle ref` in the build container")
    pts32, statement = hulls()
    pts = pts32.astype(np.float64)
    zero = np.zeros(3)
    dp = ctypes.POINTER(ctypes.c_double)
    v = np.zeros((len(pts), 3)); d = np.zeros(len(pts)); nv = np.zeros(len(pts), np.int32)
    # the reference prints a debug line on some degenerate inputs; silence fd 1 while it runs
    sys.stdout.flush()
    saved = os.dup(1); devnull = os.open(os.devnull, os.O_WRONLY); os.dup2(devnull, 1)
    try:
        for i, p in enumerate(pts):
            n = ctypes.c_int()
            d[i] = ref.ref_gjk(np.ascontiguousarray(p).ctypes.data_as(dp), 6, zero.ctypes.data_as(dp), 1, v[i].ctypes.data_as(dp), ctypes.byref(n))
            nv[i] = n.value
    finally:
        os.dup2(saved, 1); os.close(devnull); os.close(saved)
    np.savez_compressed(os.path.join(os.path.dirname(__file__), "gjk_tetra_edges.npz"), pts=pts32, statement=statement, v=v, dist=d, nvrtx=nv)
    print("wrote", len(pts), "vectors; simplex sizes:", np.bincount(nv))


if __name__ == "__main__":
    main()
