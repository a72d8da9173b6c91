from .din import DIN
from .bst import BST
from .dien import DIEN
from .dsin import DSIN
